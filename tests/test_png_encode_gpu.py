"""The device PNG encoder (csrc/png_encode.hip, render.encode_png) on the GPU: exact round trips through Pillow and zlib, the segment seams, every
block type and code path shown taken from the file's own tokens, the filter rule against its numpy restatement, the size conditions, determinism,
the real grids, the stored mode read back by the device decoder, and the refusals."""
import os
import zlib

import numpy as np
import pytest
import torch

import png_encode_common as E

pytestmark = pytest.mark.gpu

SEG = 65536
STORED, FIXED, DYNAMIC = 0, 1, 2


def _encode(dev, pixels, **kw):
    """(file bytes, segment table [n, 4]) of a host image."""
    from layoutdetr_amd import render
    data, stats = render.encode_png(torch.from_numpy(np.ascontiguousarray(pixels)).to(dev), return_stats=True, **kw)
    assert data.dtype == torch.uint8 and data.device.type == 'cpu' and data.ndim == 1
    return data.numpy().tobytes(), stats['segments']


def _check(dev, pixels, **kw):
    """Encode, check the whole-file contract and the table against the file -> (file, table, filtered stream)."""
    from layoutdetr_amd import render
    data, table = _encode(dev, pixels, **kw)
    stream = E.check_file(data, pixels)
    H, W, _ = pixels.shape
    segs = render.png_encode_segments(H, W)
    idats = [(t, d) for t, d, _ in E.chunks(data) if t == b'IDAT']
    assert len(idats) == len(segs) == len(table)                                        # one IDAT chunk per segment
    assert [(int(r[0]), int(r[1])) for r in table] == segs
    assert [int(r[3]) for r in table] == [12 + len(d) for _, d in idats]
    forced = kw.get('blocks', 'auto')
    if forced != 'auto':
        assert set(int(r[2]) for r in table) == {('stored', 'fixed', 'dynamic').index(forced)}
    return data, table, stream


@pytest.mark.parametrize('blocks', ['auto', 'stored', 'fixed', 'dynamic'])
@pytest.mark.parametrize('size', [(1, 1), (1, 5), (5, 1), (2, 3), (3, 2), (21, 1), (65, 130)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_round_trip_is_exact(dev, size, blocks):
    W, H = size
    for px in (E.noise(H, W, seed=W * 31 + H), E.flat_layout(max(H, 16), max(W, 16))[:H, :W].copy()):
        _check(dev, px, blocks=blocks)


def test_seams(dev):
    from layoutdetr_amd import render
    cases = {'one byte short of a seam': (28, 771), 'exactly at a seam': (21, 1024), 'one row past a seam': (21, 1025), 'three segments, the last a single row': (21, 2049)}
    want = {'one byte short of a seam': [(0, SEG - 1)], 'exactly at a seam': [(0, SEG)], 'one row past a seam': [(0, SEG), (SEG, SEG + 64)],
            'three segments, the last a single row': [(0, SEG), (SEG, 2 * SEG), (2 * SEG, 2 * SEG + 64)]}
    for name, (W, H) in cases.items():
        assert render.png_encode_segments(H, W) == want[name], name
        px = E.glyphs(H, W, seed=H)
        for blocks in ('auto', 'stored', 'fixed', 'dynamic'):
            _check(dev, px, blocks=blocks)
    # runs that meet the seams: all white across three segments
    px = E.white(2100, 21)
    assert len(render.png_encode_segments(2100, 21)) == 3
    data, table, _ = _check(dev, px)
    assert len(data) < 2100 * 64 // 50
    for blk in E.deflate_blocks(E.idat(data)):                                          # no match reaches back over a segment start
        at = 0
        for tok in blk.get('tokens', []):
            assert tok[0] == 'L' or tok[2] <= at, (tok, at)
            at += 1 if tok[0] == 'L' else tok[1]


def test_auto_takes_each_block_type_and_says_so(dev):
    seen = {}
    for name, px in (('noise', E.noise(100, 300)), ('short flat rows', E.flat_layout(16, 21)), ('smooth', E.photo(120, 200))):
        data, table, _ = _check(dev, px)
        types = [int(r[2]) for r in table]
        blocks = [b for b in E.deflate_blocks(E.idat(data)) if not (b['type'] == 0 and b.get('n_stored') == 0)]      # without the empty closing blocks
        assert [b['type'] for b in blocks] == [t for t, r in zip(types, table) for _ in range(1 if t else -(-int(r[1] - r[0]) // 65535))], name
        seen[name] = set(types)
    assert seen == {'noise': {STORED}, 'short flat rows': {FIXED}, 'smooth': {DYNAMIC}}, seen


def test_fixed_codes_with_nine_bit_literals(dev):
    px = np.random.RandomState(5).randint(144, 256, size=(40, 40, 3)).astype(np.uint8)
    data, table, stream = _check(dev, px, blocks='fixed', filter=0)
    blk = E.deflate_blocks(E.idat(data))[0]
    lits = [t for t in blk['tokens'] if t[0] == 'L']
    assert blk['type'] == 1 and sum(1 for t in lits if t[1] >= 144) > 4000
    assert len(E.idat(data)) > len(stream) * 1.1                                        # 9 bits per literal


def test_runs_of_every_length(dev):
    vals, v = [], 0
    for n in range(3, 301):
        vals += [v % 251] * n + [(v * 7 + 1) % 256, (v * 13 + 2) % 256]
        v += 1
    px = E.from_bytes(vals, 16000)                                                      # one row: no filter byte inside a run
    for blocks in ('fixed', 'dynamic', 'auto'):
        data, _, _ = _check(dev, px, blocks=blocks, filter=0)
        lens = set()
        for blk in E.deflate_blocks(E.idat(data)):
            lens |= {t[1] for t in blk.get('tokens', []) if t[0] == 'M'}
        assert 258 in lens and max(lens) == 258 and min(lens) == 3
        classes = {next(k for k in range(28, -1, -1) if E._LBASE[k] <= n) for n in lens}
        assert classes == set(range(29)), sorted(set(range(29)) - classes)             # every length code 257 .. 285


def test_dynamic_block_without_a_match_and_with_one_distance(dev):
    data, _, _ = _check(dev, E.noise(3, 5, seed=9), blocks='dynamic', filter=0)
    blk = E.deflate_blocks(E.idat(data))[0]
    assert blk['type'] == 2 and all(t[0] == 'L' for t in blk['tokens'])
    assert sorted(n for n in blk['dist_lengths'] if n) == [1, 1]                        # no distance code in use: two codes of length 1 are sent
    assert blk['cl_lengths'] == [4] * 16 + [0] * 3
    px = np.zeros((1, 100, 3), np.uint8)
    px[0] = (np.arange(300).reshape(100, 3) * 37 + 11) % 256
    px[0, 50:60] = 7                                                                    # one run: distance 1 only
    data, _, _ = _check(dev, px, blocks='dynamic', filter=0)
    blk = E.deflate_blocks(E.idat(data))[0]
    assert {t[2] for t in blk['tokens'] if t[0] == 'M'} == {1}
    assert sorted(n for n in blk['dist_lengths'] if n) == [1, 1]                        # exactly one in use: a second code of length 1 beside it


def test_fibonacci_counts_reach_the_15_bit_limit(dev):
    vals = E.fibonacci_bytes(16)                                                        # no three bytes repeat at the short candidate distances
    assert len(set(vals.tolist())) == 16 and len(vals) < 7000 and len(vals) % 3 == 0
    data, _, _ = _check(dev, E.from_bytes(vals, len(vals) // 3), blocks='dynamic', filter=0)      # one row: no previous-row candidate, no padding
    blk = E.deflate_blocks(E.idat(data))[0]
    lit = [n for n in blk['lit_lengths'] if n]
    lits = np.bincount([t[1] for t in blk['tokens'] if t[0] == 'L'], minlength=256)
    counts = np.bincount(vals)
    assert sorted(lits[lits > 0].tolist()) == [1] + sorted(counts[counts > 0].tolist()) and all(t[0] == 'L' for t in blk['tokens'])      # no match was found: 1 (the filter byte), 2, 3, 5, ...
    hist = np.zeros(286, np.int64)                                                      # the block's literal / length histogram, from its own tokens
    hist[256] = 1
    for t in blk['tokens']:
        hist[t[1] if t[0] == 'L' else 257 + max(k for k in range(29) if E._LBASE[k] <= t[1])] += 1
    assert E.huffman_depth(hist) > 15                                                   # an unlimited code of these counts does not fit
    assert max(lit) <= 15 and len(lit) == int((hist > 0).sum())
    assert sum(2.0 ** -n for n in lit) == 1.0                                           # rebuilt, not cut: the code is complete


FILTER_FIXTURES = {'gradient': lambda: E.gradient(40, 70), 'glyphs': lambda: E.glyphs(64, 90), 'smooth': lambda: E.photo(50, 70), 'noise': lambda: E.noise(12, 33, seed=4),
                   'flat': lambda: E.flat_layout(48, 60)}


def test_filter_bytes_are_the_rule(dev):
    seen = set()
    for name, make in FILTER_FIXTURES.items():
        px = make()
        _, _, stream = _check(dev, px)
        types, want = E.filter_choice(px)
        H, W, _ = px.shape
        got = np.frombuffer(stream, np.uint8).reshape(H, 1 + 3 * W)[:, 0]
        assert np.array_equal(got, types), (name, got.tolist(), types.tolist())
        assert stream == want, name
        seen |= set(int(t) for t in types)
    assert seen == {0, 1, 2, 3, 4}, seen
    px = E.photo(50, 70)
    for k in range(5):
        _, _, stream = _check(dev, px, filter=k)
        assert stream == E.P.filter_rows(px, (k,))


def test_size_conditions(dev, capsys):
    from layoutdetr_amd import render
    px = E.noise(384, 384)
    data, _, _ = _check(dev, px)
    bound, _ = render.png_encode_bound(384, 384)
    raw = 384 * (1 + 3 * 384)
    assert len(data) <= bound <= 1.002 * raw + 1024
    data, _, _ = _check(dev, E.white(512, 512))
    assert len(data) < 512 * (1 + 3 * 512) / 50
    ratios = {}
    for name, px in (('flat layout', E.flat_layout(384, 384)), ('glyph-like', E.glyphs(384, 384)), ('photo-like', E.photo(384, 384))):
        data, _, stream = _check(dev, px)
        deflate = len(E.idat(data)) - 6                                                 # without the zlib header and the Adler-32
        ratios[name] = deflate / len(zlib.compress(stream, 1))
    with capsys.disabled():
        print('\n[png encode] deflate bytes / len(zlib.compress(filtered, 1)): ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    for name, r in ratios.items():
        assert r <= 1.5, (name, r)


def test_two_calls_give_the_same_bytes(dev):
    px = E.glyphs(300, 200)
    assert _encode(dev, px)[0] == _encode(dev, px)[0]


def test_non_contiguous_grid(dev):
    from layoutdetr_amd import render
    px = E.photo(40, 60)
    wide = torch.from_numpy(np.ascontiguousarray(np.concatenate([px, px], 1))).to(dev)
    view = wide[:, 10:70]
    assert not view.is_contiguous()
    E.check_file(render.encode_png(view).numpy().tobytes(), view.cpu().numpy())


def test_real_grids_and_save_png(dev, tmp_path, monkeypatch):
    import PIL.Image
    from layoutdetr_amd import render
    g = torch.Generator().manual_seed(2)
    B, N = 5, 6
    bbox = torch.cat([torch.rand(B, N, 2, generator=g) * 0.6 + 0.2, torch.rand(B, N, 2, generator=g) * 0.3 + 0.05], -1).to(dev)
    valid = torch.ones(B, N, dtype=torch.bool)
    labels = torch.randint(0, 4, (B, N), generator=g)
    colors = [(230, 25, 75), (60, 180, 75), (0, 130, 200), (245, 130, 48)]
    layout = render.layout_grid(bbox, valid, labels, colors, (90, 120), canvas=64)
    E.check_file(render.encode_png(layout).numpy().tobytes(), layout.cpu().numpy())
    crops = [[E.noise(24, 27, seed=b * 7 + i) for i in range(2)] for b in range(2)]
    real = torch.tensor([0.5, 0.5, 0.3, 0.2]).repeat(2, 2, 1)
    fake = torch.tensor([[[0.3, 0.3, 0.4, 0.3], [0.6, 0.7, 0.5, 0.25]], [[0.5, 0.5, 0.6, 0.5], [0.2, 0.8, 0.3, 0.2]]])
    pages = render.PageSet([torch.from_numpy(E.photo(60, 45, seed=b)).to(dev) for b in range(2)])
    image = render.image_grid(fake.to(dev), real, torch.ones(2, 2, dtype=torch.bool), render.PatchSet(crops, dev), (90, 120), backgrounds=pages, canvas=64)
    E.check_file(render.encode_png(image).numpy().tobytes(), image.cpu().numpy())
    # save_png: the device encoder on request, today's Pillow file otherwise
    p_dev, p_def, p_env, p_ref = (str(tmp_path / n) for n in ('dev.png', 'default.png', 'env.png', 'ref.png'))
    render.save_png(image, p_dev, encoder='device')
    assert np.array_equal(np.array(PIL.Image.open(p_dev)), image.cpu().numpy())
    assert open(p_dev, 'rb').read() == render.encode_png(image).numpy().tobytes()
    monkeypatch.delenv('LDETR_SNAPSHOT_PNG', raising=False)
    render.save_png(image, p_def)
    PIL.Image.fromarray(image.cpu().numpy(), 'RGB').save(p_ref)
    assert open(p_def, 'rb').read() == open(p_ref, 'rb').read()
    monkeypatch.setenv('LDETR_SNAPSHOT_PNG', 'device')
    render.save_png(image, p_env)
    assert open(p_env, 'rb').read() == open(p_dev, 'rb').read()


def test_stored_mode_is_read_back_by_the_device_decoder(dev):
    from layoutdetr_amd.training.dataset_layoutganpp import decode_pages, scan_png
    for px in (E.photo(70, 100), E.glyphs(700, 40)):                                    # one segment; three segments, two stored blocks in each full one
        data, table, _ = _check(dev, px, blocks='stored')
        assert all(b['type'] == 0 and b['n_stored'] > 0 for b in E.deflate_blocks(E.idat(data)))      # no empty closing blocks
        raw = scan_png(data, verify=True)
        assert raw is not None and (raw.width, raw.height) == (px.shape[1], px.shape[0])
        assert np.array_equal(decode_pages([raw], dev)[0].cpu().numpy(), px)


def test_refusals(dev):
    import ctypes
    from layoutdetr_amd import _lib, render
    from layoutdetr_amd.hip import core
    with pytest.raises(RuntimeError, match='GPU'):
        render.encode_png(torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match='uint8'):
        render.encode_png(torch.zeros(4, 4, 3, device=dev))
    with pytest.raises(ValueError, match='uint8'):
        render.encode_png(torch.zeros(4, 4, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='16384'):
        render.encode_png(torch.zeros(1, 16385, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='16384'):
        render.encode_png(torch.zeros(16385, 1, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='blocks'):
        render.encode_png(torch.zeros(4, 4, 3, dtype=torch.uint8, device=dev), blocks='best')
    with pytest.raises(ValueError, match='filter'):
        render.encode_png(torch.zeros(4, 4, 3, dtype=torch.uint8, device=dev), filter=5)
    # the C entry: an output buffer one byte below the bound is refused before any launch
    H, W = 8, 8
    bound, ws_bytes = render.png_encode_bound(H, W)
    src = torch.zeros(H, W, 3, dtype=torch.uint8, device=dev)
    out = torch.full((bound,), 0xEE, dtype=torch.uint8, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    total = torch.full((1,), -7, dtype=torch.int64, device=dev)
    a = _lib.PngEncodeArgs(struct_bytes=ctypes.sizeof(_lib.PngEncodeArgs), H=H, W=W, blocks=0, filter=-1, reserved=0, src=src.data_ptr(), out=out.data_ptr(),
                           out_capacity=bound - 1, total_bytes=total.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws_bytes, seg_table=None, seg_table_rows=0)
    assert core.lib().ldetr_png_encode_u8(ctypes.byref(a), core.stream()) == 1
    assert 'output buffer' in _lib.load().ldetr_last_error().decode()
    a.out_capacity, a.workspace_bytes = bound, ws_bytes - 1
    assert core.lib().ldetr_png_encode_u8(ctypes.byref(a), core.stream()) == 1
    a.workspace_bytes, a.W = ws_bytes, 16385
    assert core.lib().ldetr_png_encode_u8(ctypes.byref(a), core.stream()) == 1
    torch.cuda.synchronize()
    assert int(total.item()) == -7 and bool((out == 0xEE).all())                        # nothing was launched
    a.W = W
    assert core.lib().ldetr_png_encode_u8(ctypes.byref(a), core.stream()) == 0
    n = int(total.item())
    E.check_file(out[:n].cpu().numpy().tobytes(), np.zeros((H, W, 3), np.uint8))
