"""The device PNG encoder, the part that needs no GPU: the ABI bookkeeping, the drop-in flag, the environment switch of save_png, the arithmetic of
png_encode_bound / png_encode_segments, and the test helpers themselves against zlib and Pillow."""
import ctypes
import io
import os
import zlib

import numpy as np
import pytest
import torch

import png_encode_common as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_signatures_and_abi_version():
    from layoutdetr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ldetr_hip.h')).read()
    for name in ('ldetr_png_encode_bound', 'ldetr_png_encode_u8'):
        assert name in _lib.SIGNATURES
        assert f'int {name}(' in header
    assert 'typedef struct ldetr_png_encode_args {' in header
    lib = _lib.load()                                                                   # resolves both symbols, checks the six mirrored argument blocks
    assert _lib.ABI_VERSION == 25 and lib.ldetr_abi_version() == 25
    sizes = (ctypes.c_int32 * 8)(*([-1] * 8))
    lib.ldetr_struct_sizes(sizes)
    assert list(sizes)[6:] == [-1, -1]                                                  # still six entries
    assert ctypes.sizeof(_lib.PngEncodeArgs) == 24 + 8 * 8
    fields = [f for f, _ in _lib.PngEncodeArgs._fields_]
    decl = header[header.index('typedef struct ldetr_png_encode_args {'):header.index('} ldetr_png_encode_args;')]
    at = [decl.index(f' {f};') if f' {f};' in decl else decl.index(f' {f},') if f' {f},' in decl else decl.index(f', {f};') for f in fields]
    assert at == sorted(at), 'the ctypes mirror lists the fields in the header\'s order'


def test_dropin_snapshot_png_flag():
    from layoutdetr_amd import dropin
    from layoutdetr_amd.training.snapshot_images import KINDS_ENV
    for value in ('device', 'pillow'):
        env = {}
        assert dropin.parse_options([f'--snapshot-png={value}', 'train.py', '--gpus=1'], env) == ['train.py', '--gpus=1']
        assert env == {'LDETR_SNAPSHOT_PNG': value}
    env = {}
    assert dropin.parse_options(['--snapshot-png', 'device', '--dataset-mode=raw', '--image-snapshot-kinds=layouts', 'train.py'], env) == ['train.py']
    assert env == {'LDETR_SNAPSHOT_PNG': 'device', 'LDETR_DATASET_MODE': 'raw', KINDS_ENV: 'layouts'}
    with pytest.raises(SystemExit, match='snapshot-png'):
        dropin.parse_options(['--snapshot-png=gpu', 'train.py'], {})
    env = {}
    assert dropin.parse_options(['train.py', '--snapshot-png=device'], env) == ['train.py', '--snapshot-png=device'] and env == {}      # after the script: the script's own


def test_save_png_reads_the_environment(monkeypatch, tmp_path):
    from layoutdetr_amd import render
    assert render.PNG_ENV == 'LDETR_SNAPSHOT_PNG'
    grid = torch.from_numpy(E.flat_layout(20, 30))
    monkeypatch.setenv('LDETR_SNAPSHOT_PNG', 'gpu')
    with pytest.raises(ValueError, match='LDETR_SNAPSHOT_PNG'):
        render.save_png(grid, str(tmp_path / 'a.png'))
    with pytest.raises(ValueError, match='LDETR_SNAPSHOT_PNG'):
        render.save_png(grid, str(tmp_path / 'a.png'), encoder='gpu')
    assert not (tmp_path / 'a.png').exists()
    # the default and 'pillow' write today's file; an explicit encoder wins over the variable
    import PIL.Image
    ref = io.BytesIO()
    PIL.Image.fromarray(grid.numpy(), 'RGB').save(ref, format='png')
    render.save_png(grid, str(tmp_path / 'b.png'), encoder='pillow')
    monkeypatch.setenv('LDETR_SNAPSHOT_PNG', 'pillow')
    render.save_png(grid, str(tmp_path / 'c.png'))
    monkeypatch.delenv('LDETR_SNAPSHOT_PNG')
    render.save_png(grid, str(tmp_path / 'd.png'))
    for n in 'bcd':
        assert (tmp_path / f'{n}.png').read_bytes() == ref.getvalue(), n
    # the device encoder has no CPU path
    monkeypatch.setenv('LDETR_SNAPSHOT_PNG', 'device')
    with pytest.raises(RuntimeError, match='GPU'):
        render.save_png(grid, str(tmp_path / 'e.png'))
    with pytest.raises(RuntimeError, match='GPU'):
        render.encode_png(grid)


@pytest.mark.parametrize('size', [(1, 1), (21, 1024), (21, 1025), (28, 771), (384, 384), (4106, 4106), (16384, 16384), (1, 16384), (16384, 1)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_bound_and_segments_arithmetic(size):
    from layoutdetr_amd import render
    W, H = size
    total = H * (1 + 3 * W)
    segs = render.png_encode_segments(H, W)
    assert segs[0][0] == 0 and segs[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))                            # they tile the stream in order
    assert all(e - s >= 32768 for s, e in segs[:-1]) and segs[-1][1] > segs[-1][0]
    assert all(e - s == render.PNG_ENCODE_SEGMENT for s, e in segs[:-1])
    bound, ws = render.png_encode_bound(H, W)
    # signature + IHDR + IEND, per segment one chunk of stored blocks (5 bytes per 65535), the zlib header and the Adler-32
    want = 8 + 25 + 12 + 2 + 4 + sum(12 + (e - s) + 5 * -(-(e - s) // 65535) for s, e in segs)
    assert bound == want
    assert bound <= 1.002 * total + 1024
    assert ws >= total + len(segs) * (12 + render.PNG_ENCODE_SLOT)


def test_bound_refuses_sizes_outside_the_range():
    from layoutdetr_amd import _lib, render
    for H, W in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        with pytest.raises(ValueError, match='16384'):
            render.png_encode_bound(H, W)
        with pytest.raises(ValueError, match='16384'):
            render.png_encode_segments(H, W)
        out = ctypes.c_int64(0)
        assert _lib.load().ldetr_png_encode_bound(H, W, ctypes.byref(out), None) == 1
        assert 'png_encode' in _lib.load().ldetr_last_error().decode()


def test_helpers_against_zlib_and_pillow():
    """The numpy filter rule gives a stream Pillow decodes to the image; the token reader reproduces zlib's own streams."""
    import PIL.Image
    import png_decode_common as P
    from layoutdetr_amd import render
    assert render.PNG_ENCODE_SEGMENT == 65536 and render.BLOCK_NAMES == ('stored', 'fixed', 'dynamic')      # what the GPU tests' seams and type columns assume
    px = E.photo(24, 37)
    types, stream = E.filter_choice(px)
    assert len(set(types.tolist())) > 1
    data = P.png_file(37, 24, zlib.compress(stream, 6), (1 << 30,))
    assert np.array_equal(np.array(PIL.Image.open(io.BytesIO(data))), px)
    assert E.check_file(data, px) == stream
    for level, raw in ((6, E.glyphs(30, 40).tobytes()), (1, E.flat_layout(30, 40).tobytes()), (0, E.noise(5, 7).tobytes()), (9, bytes(range(256)) * 3 + b'a' * 700)):
        out = bytearray()
        for blk in E.deflate_blocks(zlib.compress(raw, level)):
            if blk['type'] == 0:
                out += raw[len(out):len(out) + blk['n_stored']]
                continue
            for t in blk['tokens']:
                if t[0] == 'L':
                    out.append(t[1])
                else:
                    for _ in range(t[1]):
                        out.append(out[-t[2]])
        assert bytes(out) == raw, level
    assert E.huffman_depth([1, 1, 2, 3, 5, 8, 13, 21]) == 7 and E.huffman_depth([5, 5, 5, 5]) == 2
    vals = E.fibonacci_bytes(16)
    counts = np.bincount(vals)
    assert E.huffman_depth([1, 1] + counts[counts > 0].tolist()) == 17 and 0 not in vals
