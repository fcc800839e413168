"""CPU tests of the `images` snapshot kinds (DESIGN.md §13 rules 8-12): the fp32 restatement of the rule against the reference fixture
(tests/golden/image_snapshot.npz, tools/gen_image_snapshot_golden.py), LayoutDataset.patch_crops against the reference-mode item, the host tables and
rectangles render.py hands the kernels against the restatement, and the entries' host validation (nothing here launches a kernel)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_snapshot_common as ISC  # noqa: E402
import snapshot_common as SC  # noqa: E402

G = os.path.join(ROOT, 'tests', 'golden')
TINY = os.path.join(G, 'dataset_tiny.zip')


@pytest.fixture(scope='module')
def gold():
    d = np.load(os.path.join(G, 'image_snapshot.npz'), allow_pickle=False)
    return {k: d[k] for k in d.files}


def cases(gold):
    for name, (W, H, S) in zip(gold['cases'].tolist(), gold['case_whs'].tolist()):
        crops = ISC.unpack_crops(gold[f'{name}_crops'], gold[f'{name}_crop_table'])
        bgs = [gold[f'{name}_backgrounds'][b % 2] for b in range(5)]
        yield name, W, H, S, gold[f'{name}_bbox_fake'], gold[f'{name}_valid'], crops, bgs


def judge(mine, ref, keeps_size, what):
    """The two bars of DESIGN.md §13: at most 1 level anywhere (both are floors of values that agree to about 1e-3 levels, and the 8-bit bilinear tail
    cannot widen a difference of 1); where no resize keeps a size on an axis, at most 1 % of the cell's pixels differ (a cap against a systematic
    off-by-one; an fp32 emulation gave <= 0.2 %)."""
    diff = np.abs(mine.astype(np.int32) - ref.astype(np.int32))
    share = float((diff != 0).any(-1).mean())
    print(f'{what}: max difference {int(diff.max())}, differing pixels {100 * share:.3f} %' + (' (a resize keeps a size)' if keeps_size else ''))
    assert diff.max() <= 1, what
    if not keeps_size:
        assert share <= 0.01, what


def test_fixture_covers_the_case_list(gold):
    seen = set()
    for name, W, H, S, fake, valid, crops, bgs in cases(gold):
        assert [int(v.sum()) for v in valid] == [0, 1, 9, 7, 8] and valid[4, 1] == 0
        assert bgs[0].shape[0] != H and bgs[0].shape[1] != W
        for b in range(5):
            for i, crop, (x1, y1, x2, y2) in ISC.jobs_of_cell(fake[b], valid[b], crops[b], W, H):
                (h, w), (ho, wo) = crop.shape[:2], (y2 - y1, x2 - x1)
                seen.add(('y<' if ho < h else 'y>' if ho > h else 'y=') + ('x<' if wo < w else 'x>' if wo > w else 'x='))
                seen.update(k for k, c in (('one row out', ho == 1), ('3 to 1', (w, wo) == (3, 1)), ('one column in', w == 1), ('off left', x1 < 0),
                                           ('off right', x2 > W), ('off top', y1 < 0), ('off bottom', y2 > H)) if c)
        a = fake[3, :4, 2] * fake[3, :4, 3]
        assert (a == a[0]).all() and valid[3, :4].all()                           # equal fp32 areas: the tie order decides
        undrawn = [paste for paste in (ISC.paste_rect(fake[4, i], W, H) for i in (5, 6, 7, 8))]
        assert undrawn[0][0] >= W and undrawn[1][2] <= 0 and undrawn[2][3] <= 0 and undrawn[3][1] >= H       # wholly off the page, each side
        # the fixture's own noise floor (its two reference runs against each other) off the identity cell: what the generator asserted
        assert (gold[f'{name}_white_noise'][[0, 2, 3, 4]] <= 0.0025).all() and (gold[f'{name}_bg_noise'][[0, 2, 3, 4]] <= 0.0025).all()
    assert {'y<x<', 'y>x>', 'y<x>', 'y>x<', 'y=x=', 'one row out', '3 to 1', 'one column in', 'off left', 'off right', 'off top', 'off bottom'} <= seen


def test_fp32_rule_matches_the_reference_cells(gold):
    for name, W, H, S, fake, valid, crops, bgs in cases(gold):
        for tag, backs in (('white', [None] * 5), ('bg', bgs)):
            for b in range(5):
                mine = ISC.cell_f32(fake[b], valid[b], crops[b], W, H, S, backs[b])
                keeps = ISC.keeps_a_size(fake[b], valid[b], crops[b], W, H, backs[b])
                judge(mine, gold[f'{name}_{tag}'][b], keeps, f'{name} {tag} cell {b}')
                # the float64-input run of the reference (stored as its XOR with the first) under the same bars
                judge(mine, gold[f'{name}_{tag}'][b] ^ gold[f'{name}_{tag}_exact_xor'][b], keeps, f'{name} {tag} cell {b} (float64 inputs)')
    assert (gold['land_white'][0] == ISC.letterbox(np.full((30, 50, 3), 255, np.uint8), 40)).all()        # nothing valid: the white page


def test_identity_size_jobs_return_the_crop(gold):
    rng = np.random.RandomState(5)
    crops = [c for _, _, _, _, _, _, cc, _ in cases(gold) for row in cc for c in row if c is not None]
    assert len(crops) > 50
    for c in crops + [rng.randint(0, 256, size=(7, 1, 3)).astype(np.uint8), np.arange(256 * 3, dtype=np.uint8).reshape(1, 256, 3)]:
        assert np.array_equal(ISC.resize_f32(c, c.shape[0], c.shape[1]), c)
    # the same through a page: cell 1 of every case pastes its crop unchanged
    for name, W, H, S, fake, valid, crops, bgs in cases(gold):
        (i, crop, (x1, y1, x2, y2)), = ISC.jobs_of_cell(fake[1], valid[1], crops[1], W, H)
        assert np.array_equal(ISC.page_f32(fake[1], valid[1], crops[1], W, H)[y1:y2, x1:x2], crop)


def test_tiny_items_through_patch_crops(gold):
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset
    dev, ref = LayoutDataset(TINY, mode='device'), LayoutDataset(TINY, mode='reference')
    try:
        drawn = 0
        S = int(gold['tiny_canvas'])
        for b in range(len(dev)):
            item, crops = ref[b][0], dev.patch_crops(b)
            before = dev[b][0]
            assert sorted(before) == sorted(dev[b][0]) and 'patches_orig' not in before              # __getitem__ is unchanged
            W, H = int(item['W_page']), int(item['H_page'])
            assert len(crops) == 9 and (W, H) == tuple(gold['tiny_wh'][b])
            for k in range(9):
                if not item['mask'][k]:
                    assert crops[k] is None
                    continue
                # the crop the reference takes from the normalised canvas (util.py:159-164), de-normalised
                canvas = np.transpose(np.asarray(item['patches_orig'][k]), [1, 2, 0])
                win = ISC.crop_window(canvas.shape[:2], item['bboxes'][k], W, H)
                if win is None:
                    assert crops[k] is None
                    continue
                im = np.clip(canvas[win[0]:win[1], win[2]:win[3]] * ISC.RGB_STD + ISC.RGB_MEAN, 0.0, 1.0)
                assert crops[k].dtype == np.uint8 and np.array_equal(crops[k], np.rint(im.astype(np.float64) * 255.0).astype(np.uint8))
                drawn += 1
            valid = np.asarray(item['mask']).astype(np.uint8)
            mine = ISC.cell_f32(gold['tiny_bbox_fake'][b], valid, crops, W, H, S)
            judge(mine, gold['tiny_white'][b], ISC.keeps_a_size(gold['tiny_bbox_fake'][b], valid, crops, W, H), f'tiny item {b}')
        assert drawn >= 1
    finally:
        dev.close(); ref.close()


def test_host_tables_and_rectangles_match_the_restatement(gold):
    from layoutdetr_amd import render
    for n_in, n_out in [(5, 5), (3, 1), (1, 4), (59, 35), (12, 9), (7, 30), (200, 3)]:
        words = render.resize_axis_table(n_in, n_out)
        r, g, i0, i1, w0, w1 = ISC.axis_table(n_in, n_out)
        mine = np.concatenate([np.asarray([r], np.int32), g.astype(np.float32).view(np.int32), i0.astype(np.int32), i1.astype(np.int32),
                               w0.astype(np.float32).view(np.int32), w1.astype(np.float32).view(np.int32)])
        assert words.dtype == np.int32 and np.array_equal(words, mine)
        assert 0 <= i0.min() and i1.max() < n_in and abs(float(g.sum()) - 1) < 1e-12
    assert ISC.axis_table(3, 1)[0] == 4 and ISC.axis_table(5, 5)[0] == 0
    for name, W, H, S, fake, valid, crops, bgs in cases(gold):
        rects = render.paste_rects(fake, [(W, H)] * 5)
        for b in range(5):
            for i in range(9):
                assert tuple(rects[b, i]) == ISC.paste_rect(fake[b, i], W, H)
    nan = np.asarray([[[np.nan, 0.5, 0.2, 0.2], [0.5, 0.5, 0.25, 0.25]]], np.float32)
    assert render.paste_rects(nan, (8, 8)).tolist() == [[[0, 0, 0, 0], [3, 3, 5, 5]]] and ISC.paste_rect(nan[0, 0], 8, 8) is None
    # the tail is layout_grid's: one cell_size / grid_shape for both kinds of grid
    assert render.cell_size(50, 30, 40) == SC.cell_size(50, 30, 40) and render.grid_shape(5, 40, 3) == (2 * 42 + 2, 3 * 42 + 2, 3, 2)
    assert render.IMAGE_CANVAS == 1024


def test_kinds_are_opt_in():
    from layoutdetr_amd.training import snapshot_images as SI
    assert SI.DEFAULT_KINDS == ('layouts', 'layouts_over_background') and SI.parse_kinds(None) == SI.DEFAULT_KINDS == SI.parse_kinds('')
    assert SI.parse_kinds('images_with_background, layouts,images') == ('layouts', 'images', 'images_with_background')
    assert SI.parse_kinds(['images']) == ('images',)
    with pytest.raises(ValueError, match='unknown image snapshot kind'):
        SI.parse_kinds('layouts,pictures')


def test_launcher_option_names_the_kinds(tmp_path, monkeypatch):
    """`python -m layoutdetr_amd.dropin --image-snapshot-kinds=... script.py args`: the kinds reach training_loop through the environment."""
    from layoutdetr_amd import dropin
    from layoutdetr_amd.training.snapshot_images import KINDS_ENV
    script = tmp_path / 'probe.py'
    script.write_text('import os, sys\nopen(sys.argv[1], "w").write(os.environ.get(%r, "") + " " + str(len(sys.argv)))\n' % KINDS_ENV)
    monkeypatch.delenv(KINDS_ENV, raising=False)
    saved_argv, saved_path = list(sys.argv), list(sys.path)
    try:
        dropin.main(['--image-snapshot-kinds=images,layouts', str(script), str(tmp_path / 'out.txt')])
        with pytest.raises(ValueError, match='unknown image snapshot kind'):
            dropin.main(['--image-snapshot-kinds', 'pictures', str(script)])
    finally:
        dropin.uninstall()
        sys.argv[:], sys.path[:] = saved_argv, saved_path
        os.environ.pop(KINDS_ENV, None)
    assert (tmp_path / 'out.txt').read_text() == 'layouts,images 2'


def test_no_cpu_fallback():
    from layoutdetr_amd import render
    b = torch.zeros(1, 2, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        render.image_grid(b, b, torch.ones(1, 2), None, (8, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        render.PatchSet([[np.zeros((2, 2, 3), np.uint8)]], 'cpu')


def _resize_args(jobs, tables, src_bytes=1000, dst_bytes=1000):
    from layoutdetr_amd import _lib
    a = _lib.PatchResizeArgs()
    a.struct_bytes, a.n_jobs = ctypes.sizeof(_lib.PatchResizeArgs), len(jobs)
    a.src0, a.src0_bytes, a.dst, a.dst_bytes = 0x1000, src_bytes, 0x1000, dst_bytes            # never dereferenced: every call below fails before the launch
    a.jobs, a.tables, a.tables_host, a.tables_len, a.jobs_dev = jobs.ctypes.data, 0x1000, tables.ctypes.data, tables.size, 0x1000
    return a


def test_entries_validate_on_the_host_before_any_launch():
    from layoutdetr_amd import _lib, render
    lib = _lib.load()

    def resize_fails(match, jobs, tables, **kw):
        jobs = np.ascontiguousarray(np.asarray(jobs, np.int64).reshape(-1, 9))
        a = _resize_args(jobs, tables, **kw)
        with pytest.raises(RuntimeError, match=match):
            _lib.check(lib.ldetr_patch_resize_u8(ctypes.byref(a), None), 'patch_resize')
    ty, tx = render.resize_axis_table(6, 4), render.resize_axis_table(5, 8)
    pool = np.ascontiguousarray(np.concatenate([ty, tx]))
    good = [0, 0, 6, 5, 0, 4, 8, 0, ty.size]
    resize_fails('source reaches past its buffer', good, pool, src_bytes=6 * 5 * 3 - 1)
    resize_fails('target reaches past the output buffer', good, pool, dst_bytes=4 * 8 * 3 - 1)
    resize_fails('source buffer 1 is null', [1] + good[1:], pool)
    resize_fails('table offset outside the pool', good[:8] + [pool.size], pool)
    resize_fails('table reaches past the pool', good, pool[:-1].copy())
    resize_fails(r'outside \[1, 16384\]', [0, 0, 6, 5, 0, 0, 8, 0, ty.size], pool)
    bad = pool.copy(); bad[ty.size + 2 + 2 * int(tx[0])] = 5                                   # an i0 of the axis-1 table names column 5 of 5
    resize_fails('names source index 5 of 5', good, bad)
    # one output pixel whose source window cannot fit the LDS buffers: 4000 x 4000 -> 100 x 100 (radius 78 on both axes: 158 x 158 pixels)
    big = render.resize_axis_table(4000, 100)
    resize_fails('more than the 10240 floats of LDS', [0, 0, 4000, 4000, 0, 100, 100, 0, 0], big, src_bytes=4000 * 4000 * 3, dst_bytes=100 * 100 * 3)
    a = _resize_args(np.zeros((1, 9), np.int64), pool)
    a.struct_bytes -= 8
    with pytest.raises(RuntimeError, match='argument block'):
        _lib.check(lib.ldetr_patch_resize_u8(ctypes.byref(a), None), 'patch_resize')

    def raster(N=2, S=8, pixels_bytes=1000, rect=(1, 1, 5, 4), patch_off=0, page_off=-1, coeff=(0, 3, 100, 3), wh=(16, 8)):
        keep = [np.ones((1, N), np.uint8), np.asarray([rect] * N, np.int32).reshape(1, N, 4).copy(), np.full((1, N), patch_off, np.int64),
                np.asarray([page_off], np.int64), np.asarray([wh], np.int32), np.asarray([coeff], np.int64)]
        a = _lib.ImageRasterArgs()
        a.struct_bytes = ctypes.sizeof(_lib.ImageRasterArgs)
        a.B, a.N, a.S, a.nrow = 1, N, S, 0
        a.bbox, a.pixels, a.coeffs, a.cells_dev, a.out = 0x1000, 0x1000, 0x1000, 0x1000, 0x1000
        a.valid, a.rects, a.patch_off, a.page_off, a.page_wh, a.cell_coeffs = (k.ctypes.data for k in keep)
        a.pixels_bytes, a.coeffs_len = pixels_bytes, 1000
        return a, keep

    def raster_fails(match, **kw):
        a, keep = raster(**kw)
        with pytest.raises(RuntimeError, match=match):
            _lib.check(lib.ldetr_image_raster_u8(ctypes.byref(a), None), 'image_raster')
    raster_fails('1 <= N <= 16', N=17)
    raster_fails('canvas size must be even', S=7)
    raster_fails('resized patch of slot 0 reaches past the pixel buffer', pixels_bytes=4 * 3 * 3 - 1)
    raster_fails('resized patch of slot 0 reaches past the pixel buffer', patch_off=-1)
    raster_fails('resized background reaches past the pixel buffer', page_off=1000 - 16 * 8 * 3 + 1)
    raster_fails('horizontal coefficient table outside the pool', coeff=(990, 3, 100, 3))
    raster_fails('bad page size', wh=(0, 8))
