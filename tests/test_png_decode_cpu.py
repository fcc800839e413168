"""Stored-block PNG pages, the part that needs no GPU: the test writer (tests/png_decode_common.py) against Pillow, `ldetr_png_scan` against a
plain-Python walk, its three outcomes, `scan_png(verify=True)`, LayoutDataset(mode='raw'), `collate`, the ABI bookkeeping and the drop-in flag."""
import ctypes
import io
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import png_decode_common as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZIP = os.path.join(ROOT, 'tests', 'golden', 'dataset_tiny.zip')

# (W, H, schedule, layout): every layout, zero-length and 1-byte blocks, block headers split over 1-7-byte chunks, Average rows, a 1 x 1 page
WRITER_CASES = [(1, 1, 'all_0', 'one_block_one_chunk'), (1, 1, 'all_4', 'blocks_0_5_1_0_17_chunks_1_2_7_4'), (1, 5, 'random_mix', 'blocks_1_chunks_3'),
                (2, 3, 'all_3', 'blocks_0_5_1_0_17_chunks_1_2_7_4'), (7, 7, 'random_mix', 'blocks_1_chunks_3'), (7, 7, 'all_3', 'ancillary'),
                (80, 56, 'random_mix', 'pillow_65535_65536'), (80, 56, 'all_4', 'blocks_0_5_1_0_17_chunks_1_2_7_4'), (63, 64, 'all_2', 'one_block_one_chunk'),
                (65, 65, 'row0_4_then_1', 'blocks_1_chunks_3'), (40, 130, 'row0_3_then_0', 'ancillary'), (257, 129, 'random_mix', 'pillow_65535_65536')]


def _file(W, H, sched, layout):
    px, files = P.case_files(W, H, sched)
    return px, files[layout]


def _scan_raw(data, seg_capacity=None):
    """(rc, width, height, channels, segments, row_starts) straight from the C entry."""
    from layoutdetr_amd import _lib
    lib = _lib.load()
    arr = np.frombuffer(data, np.uint8)
    w, h, c, k, r = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    src = arr.ctypes.data_as(ctypes.c_void_p)
    rc = lib.ldetr_png_scan(src, arr.size, ctypes.byref(w), ctypes.byref(h), ctypes.byref(c), None, 0, ctypes.byref(k), None, 0, ctypes.byref(r))
    if rc != 0:
        return rc, w.value, h.value, c.value, None, None
    seg = np.zeros((k.value if seg_capacity is None else seg_capacity, 3), np.int64)
    rows = np.zeros(r.value, np.int32)
    rc = lib.ldetr_png_scan(src, arr.size, ctypes.byref(w), ctypes.byref(h), ctypes.byref(c), seg.ctypes.data_as(ctypes.c_void_p), len(seg), ctypes.byref(k),
                            rows.ctypes.data_as(ctypes.c_void_p), len(rows), ctypes.byref(r))
    return rc, w.value, h.value, c.value, seg[:k.value], rows


def _err():
    from layoutdetr_amd import _lib
    return _lib.load().ldetr_last_error().decode()


@pytest.mark.parametrize('case', WRITER_CASES, ids=lambda c: f'{c[0]}x{c[1]}-{c[2]}-{c[3]}')
def test_writer_decodes_in_pillow_and_scan_equals_python_walk(case):
    px, data = _file(*case)
    assert np.array_equal(P.pillow_decode(data), px)
    rc, w, h, c, seg, rows = _scan_raw(data)
    assert (rc, w, h, c) == (0, case[0], case[1], 3)
    want = P.python_walk(data)
    assert [tuple(int(v) for v in s) for s in seg] == want
    assert sum(s[2] for s in want) == h * (1 + 3 * w)
    assert rows[0] == 0 and np.all(np.diff(rows) >= 64) and np.all(rows < h)
    filt = P.filter_rows(px, P.schedules(h, case[0] + case[1])[case[2]])
    assert all(filt[int(y) * (1 + 3 * w)] <= 1 for y in rows[1:])          # a listed row reads nothing above it


def test_two_call_capacity_protocol():
    _, data = _file(7, 7, 'random_mix', 'blocks_1_chunks_3')
    rc, _, _, _, seg, _ = _scan_raw(data)
    assert rc == 0 and len(seg) == 7 * 22                                     # the null-table call returned the count the second call filled
    rc = _scan_raw(data, seg_capacity=len(seg) - 1)[0]
    assert rc == 1 and 'too small' in _err()                                  # LDETR_ERR_ARG: neither "not eligible" nor "malformed"


def _pil_bytes(im, **kw):
    buf = io.BytesIO()
    im.save(buf, format='png', **kw)
    return buf.getvalue()


def test_not_eligible_kinds():
    import PIL.Image
    from layoutdetr_amd.training.dataset_layoutganpp import scan_png
    rgb = P.noise_page(9, 6, 1)
    im = PIL.Image.fromarray(rgb)
    px, stored = _file(9, 6, 'all_1', 'one_block_one_chunk')
    H, W, _ = px.shape
    z = P.stored_zlib(P.filter_rows(px, (0,)), (65535,))
    cases = {
        'compress_level_6': _pil_bytes(PIL.Image.fromarray(np.full((6, 9, 3), 200, np.uint8)), compress_level=6),      # (zlib stores noise as it is: a flat page compresses)
        'interlaced': P.png_file(W, H, z, (1 << 30,), interlace=1),            # (Pillow cannot write Adam7; the header is what the scan reads)
        'palette': _pil_bytes(im.convert('P'), compress_level=0),
        '16_bit': _pil_bytes(PIL.Image.fromarray((rgb[:, :, 0].astype(np.uint16) << 8)), compress_level=0),
        'L': _pil_bytes(im.convert('L'), compress_level=0),
        'RGBA': _pil_bytes(im.convert('RGBA'), compress_level=0),
        'preset_dictionary': P.png_file(W, H, b'\x78\x20' + z[2:], (1 << 30,)),
    }
    assert scan_png(stored) is not None
    for name, data in cases.items():
        rc = _scan_raw(data)[0]
        assert rc == 3, (name, rc, _err())                                      # LDETR_PNG_NOT_ELIGIBLE
        assert _err(), name
        assert scan_png(data) is None, name
    # what Pillow itself saves the way dataset_tool.py does is eligible
    assert scan_png(_pil_bytes(im, compress_level=0, optimize=False)) is not None


def test_malformed_kinds():
    from layoutdetr_amd.training.dataset_layoutganpp import scan_png
    px, good = _file(9, 6, 'all_1', 'one_block_one_chunk')
    H, W, _ = px.shape
    stream = P.filter_rows(px, (1,))
    z = P.stored_zlib(stream, (65535,))
    bad_nlen = bytearray(z); bad_nlen[5] ^= 0x01                                # the NLEN of the first block
    five = bytearray(stream); five[2 * (1 + 3 * W)] = 5
    cases = {
        'truncated': good[:len(good) - 40],
        'truncated_in_signature': good[:5],
        'bad_signature': b'\x89PNX' + good[4:],
        'chunk_length_past_end': good[:33] + struct.pack('>I', 1 << 20) + good[37:],
        'wrong_nlen': P.png_file(W, H, bytes(bad_nlen), (1 << 30,)),
        'short_payload': P.png_file(W, H, P.stored_zlib(stream[:-1], (65535,)), (1 << 30,)),
        'long_payload': P.png_file(W, H, P.stored_zlib(stream + b'\x00', (65535,)), (1 << 30,)),
        'filter_byte_5': P.png_file(W, H, P.stored_zlib(bytes(five), (65535,)), (1 << 30,)),
        'missing_iend': P.png_file(W, H, z, (1 << 30,), iend=False),
    }
    for name, data in cases.items():
        rc = _scan_raw(data)[0]
        assert rc == 4, (name, rc, _err())                                      # LDETR_PNG_MALFORMED
        assert _err().startswith('png_scan:'), name
        with pytest.raises(ValueError, match='png_scan'):
            scan_png(data)


def test_verify_catches_one_flipped_payload_byte():
    from layoutdetr_amd.training.dataset_layoutganpp import scan_png
    px, good = _file(80, 56, 'random_mix', 'pillow_65535_65536')
    raw = scan_png(good, verify=True)
    assert (raw.width, raw.height) == (80, 56)
    bad = bytearray(good)
    o, _, n = raw.segments[0]
    bad[int(o) + 1 + 7] ^= 0x10                                                  # a pixel byte of row 0, not a filter byte
    assert scan_png(bytes(bad)) is not None                                     # the structure is intact: the plain scan does not look at checksums
    with pytest.raises(ValueError, match='CRC-32'):
        scan_png(bytes(bad), verify=True)
    # the chunk CRC repaired, the Adler-32 still that of the original payload
    pos = 8
    while bad[pos + 4:pos + 8] != b'IDAT':
        pos += 12 + struct.unpack('>I', bad[pos:pos + 4])[0]
    n = struct.unpack('>I', bad[pos:pos + 4])[0]
    bad[pos + 8 + n:pos + 12 + n] = struct.pack('>I', zlib.crc32(bytes(bad[pos + 4:pos + 8 + n])))
    with pytest.raises(ValueError, match='Adler-32'):
        scan_png(bytes(bad), verify=True)
    with pytest.raises(Exception):
        P.pillow_decode(bytes(bad))                                              # Pillow refuses it too


def test_raw_mode_on_the_fixture_all_items_raw_and_device_mode_unchanged():
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset, RawPage
    dev_ds = LayoutDataset(path=ZIP, background_size=32, mode='device')
    raw_ds = LayoutDataset(path=ZIP, background_size=32, mode='raw')
    assert len(raw_ds) == len(dev_ds) == 3
    filters = set()
    for i in range(3):
        (a, la), (b, lb) = dev_ds[i], raw_ds[i]
        assert isinstance(a['background'], np.ndarray) and a['background'].dtype == np.uint8 and a['background'].shape == (56, 80, 3)
        assert sorted(a) == sorted(b) and np.array_equal(la, lb)
        for k in a:
            if k == 'background':
                continue
            assert (a[k] == b[k]) if isinstance(a[k], (str, list, int, float)) else np.array_equal(a[k], b[k]), k
        page = b['background']
        assert isinstance(page, RawPage) and page.shape == a['background'].shape
        assert np.array_equal(P.pillow_decode(page.data.tobytes()), a['background'])          # the file bytes, untouched
        assert int(page.segments[:, 2].sum()) == 56 * (1 + 3 * 80)
        filters |= {int(page.data[int(page.segments[0, 0])])}
    assert raw_ds.route_counts == {'raw': 3, 'decoded': 0}
    assert dev_ds.route_counts == {'raw': 0, 'decoded': 0}


def test_raw_getitem_never_touches_the_gpu_side_of_the_library(monkeypatch):
    """`__getitem__` runs in DataLoader workers: the scan must load the C library only, not register a GPU workspace (hip.core.lib does)."""
    from layoutdetr_amd.hip import core
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset, RawPage

    def boom():
        raise AssertionError('core.lib() called from the host scan')
    monkeypatch.setattr(core, 'lib', boom)
    assert isinstance(LayoutDataset(path=ZIP, mode='raw')[0][0]['background'], RawPage)


def test_default_mode_follows_the_environment(monkeypatch):
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset
    monkeypatch.delenv('LDETR_DATASET_MODE', raising=False)
    assert LayoutDataset(path=ZIP).mode == 'device'
    monkeypatch.setenv('LDETR_DATASET_MODE', 'raw')
    assert LayoutDataset(path=ZIP).mode == 'raw'
    assert LayoutDataset(path=ZIP, mode='device').mode == 'device'              # an explicit mode wins
    monkeypatch.setenv('LDETR_DATASET_MODE', 'host')
    with pytest.raises(ValueError, match='LDETR_DATASET_MODE'):
        LayoutDataset(path=ZIP)


def test_collate_raw_decoded_and_mixed():
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset, RawPage
    dev_ds = LayoutDataset(path=ZIP, background_size=32, mode='device')
    raw_ds = LayoutDataset(path=ZIP, background_size=32, mode='raw')
    d, r = [dev_ds[i] for i in range(3)], [raw_ds[i] for i in range(3)]
    sd, ld = LayoutDataset.collate(d)
    sr, lr = LayoutDataset.collate(r)
    sm, _ = LayoutDataset.collate([r[0], d[1], r[2]])
    assert torch.is_tensor(sd['background']) and sd['background'].shape == (3, 56, 80, 3)      # decoded items: one uint8 tensor, as before
    assert isinstance(sr['background'], list) and all(isinstance(p, RawPage) for p in sr['background'])
    assert [isinstance(p, RawPage) for p in sm['background']] == [True, False, True]
    assert torch.equal(sm['background'][1], sd['background'][1])
    for k in sd:
        if k == 'background':
            continue
        same = torch.equal(sd[k], sr[k]) if torch.is_tensor(sd[k]) else sd[k] == sr[k]
        assert same, k
    assert sr['patches'].stride(0) == 0 and torch.equal(ld, lr)


def test_raw_page_pin_memory_keeps_the_tables():
    from layoutdetr_amd.training.dataset_layoutganpp import RawPage
    assert callable(getattr(RawPage, 'pin_memory', None))                        # what DataLoader(pin_memory=True) looks for on a batch element
    page = RawPage(np.arange(5, dtype=np.uint8), 1, 1, np.array([[0, 0, 4]], np.int64), np.zeros(1, np.int32))
    assert torch.equal(page.tensor(), torch.arange(5, dtype=torch.uint8))


def test_decode_pages_needs_a_gpu():
    from layoutdetr_amd.training.dataset_layoutganpp import decode_pages, scan_png
    raw = scan_png(_file(2, 3, 'all_1', 'one_block_one_chunk')[1])
    with pytest.raises(RuntimeError, match='GPU'):
        decode_pages([raw], 'cpu')


def test_header_signatures_and_abi_version():
    from layoutdetr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ldetr_hip.h')).read()
    for name in ('ldetr_png_scan', 'ldetr_png_decode_u8'):
        assert name in _lib.SIGNATURES
        assert f'int {name}(' in header
    for cite in ('dataset_tool.py:325-363', 'dataset_layoutganpp.py:329-340'):
        assert header.count(cite) >= 2
    assert _lib.ABI_VERSION == 25 and _lib.load().ldetr_abi_version() == 25
    assert ctypes.sizeof(_lib.PngDecodeArgs) == 24 + 13 * 8


def test_dropin_dataset_mode_flag():
    from layoutdetr_amd import dropin
    env = {}
    assert dropin.parse_options(['--dataset-mode=raw', 'train.py', '--gpus=1'], env) == ['train.py', '--gpus=1']
    assert env == {'LDETR_DATASET_MODE': 'raw'}
    env = {}
    assert dropin.parse_options(['--dataset-mode', 'device', '--image-snapshot-kinds=layouts', 'train.py'], env) == ['train.py']
    from layoutdetr_amd.training.snapshot_images import KINDS_ENV
    assert env == {'LDETR_DATASET_MODE': 'device', KINDS_ENV: 'layouts'}
    with pytest.raises(SystemExit, match='dataset-mode'):
        dropin.parse_options(['--dataset-mode=host', 'train.py'], {})
    assert dropin.parse_options(['train.py', '--dataset-mode=raw'], env := {}) == ['train.py', '--dataset-mode=raw'] and env == {}      # after the script: the script's own
