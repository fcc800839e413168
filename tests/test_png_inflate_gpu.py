"""Indexed page PNGs decoded on the device (csrc/png_inflate.hip): render.encode_png(index=True) -> scan_png(packed=True) ->
decode_pages must give the pixels back, bit for bit what Pillow reads from the same bytes, at the smallest shapes at which each path of the kernel can
break; the ldIX chunk the device wrote must be the index of the file's own tokens.  Well-formed files only: corrupted ones go to the host build of the
kernel (test_png_inflate_cpu.py), never to a GPU."""
import io
import struct
import zipfile
import zlib

import numpy as np
import pytest
import torch

import png_encode_common as E

pytestmark = pytest.mark.gpu

SEG, SUB = 65536, 512


def _dev():
    return torch.device('cuda:0')


def _encode(px, **kw):
    from layoutdetr_amd import render
    return render.encode_png(torch.from_numpy(np.ascontiguousarray(px)).to(_dev()), index=True, **kw).numpy().tobytes()


def _decode(files):
    """decode_pages on scanned files -> (result, status tensor)."""
    from layoutdetr_amd.training.dataset_layoutganpp import PageStatus, decode_pages, scan_png
    raws = [scan_png(f, packed=True, verify=True) for f in files]
    assert all(r is not None for r in raws)
    st = PageStatus()
    out = decode_pages(raws, _dev(), status=st)
    return out, st.tensor(), raws


def expected_index(data):
    """(filter bytes, entries per segment, block types per segment, tokens per segment) of an indexed file, from its own deflate tokens: the bit offset of
    a sub-block's first token is the header's length plus the code lengths and extra bits of every token before it."""
    ch = E.chunks(data)
    W, H = struct.unpack('>II', ch[0][1][:8])
    stride, total = 1 + 3 * W, H * (1 + 3 * W)
    stream = zlib.decompress(E.idat(data))
    blocks = E.deflate_blocks(E.idat(data))
    entries, kinds, tokens, b = [], [], [], 0
    for s, a in enumerate(range(0, total, SEG)):
        n = min(SEG, total - a)
        nsub = -(-n // SUB)
        if blocks[b]['type'] == 0:
            got = 0
            while got < n:
                assert blocks[b]['type'] == 0
                got += blocks[b]['n_stored']
                b += 1
            assert got == n
            entries.append([0] * nsub)
            kinds.append(0)
            tokens.append(None)
            continue
        blk = blocks[b]
        assert blocks[b + 1]['type'] == 0 and blocks[b + 1]['n_stored'] == 0 and blocks[b + 1]['final'] == (1 if a + n == total else 0) and blk['final'] == 0
        b += 2
        lit, dist = blk['lit_lengths'], blk['dist_lengths']
        bit = (16 if s == 0 else 0) + (3 if blk['type'] == 1 else 17 + 57 + 4 * (len(lit) + len(dist)))
        es, pos = [], 0
        for t in blk['tokens']:
            if pos % SUB == 0:
                es.append(bit)
            if t[0] == 'L':
                bit += lit[t[1]]
                pos += 1
            else:
                ls = max(k for k in range(29) if E._LBASE[k] <= t[1])
                ds = max(k for k in range(30) if E._DBASE[k] <= t[2])
                bit += lit[257 + ls] + E._LEXT[ls] + dist[ds] + E._DEXT[ds]
                assert pos // SUB == (pos + t[1] - 1) // SUB and t[2] <= pos, 'a token crosses a sub-block or a match leaves its segment'
                pos += t[1]
        assert pos == n and len(es) == nsub
        entries.append(es)
        kinds.append(blk['type'])
        tokens.append(blk['tokens'])
    assert b == len(blocks)
    return bytes(stream[y * stride] for y in range(H)), entries, kinds, tokens


def check_roundtrip(px, **kw):
    """One page through encode -> scan -> decode; returns (file, block types per segment, tokens per segment)."""
    data = _encode(px, **kw)
    ch = E.chunks(data)
    assert [t for t, _, _ in ch] == [b'IHDR', b'ldIX'] + [b'IDAT'] * (len(ch) - 3) + [b'IEND']
    assert all(crc == zlib.crc32(t + d) for t, d, crc in ch)
    assert np.array_equal(E.pillow_decode(data), px)
    filters, entries, kinds, tokens = expected_index(data)
    H = px.shape[0]
    assert ch[1][1] == struct.pack('>III', 1, SEG, SUB) + filters + b''.join(struct.pack('>I', e) for es in entries for e in es)
    out, status, raws = _decode([data])
    if all(k == 0 for k in kinds):
        assert raws[0].kind == 'stored' and status.numel() == 0                         # a stored-block file: the stored path, no status
    else:
        assert raws[0].kind == 'packed' and raws[0].packed[0][:, 2].tolist() == kinds and status.tolist() == [0]
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1,) + px.shape
    assert np.array_equal(out[0].cpu().numpy(), px)
    return data, kinds, tokens


def _half_noise(H, W):
    return np.concatenate([E.noise(H // 2, W, seed=4), E.flat_layout(H - H // 2, W, seed=5)], 0)


SHAPES = {                                                                              # (H, W)
    '1x1': lambda: E.noise(1, 1),                                                       # one short sub-block
    '3x5': lambda: E.photo(5, 3),
    '1024x21_one_full_segment': lambda: E.glyphs(1024, 21),                             # rows of 64 bytes: exactly 65536
    '1025x21_second_segment_of_64': lambda: E.glyphs(1025, 21),
    '300x100_seam_mid_row': lambda: E.photo(300, 100),                                  # rows of 301 bytes: the seam mid-row, sub-block ends mid-pixel
}


@pytest.mark.parametrize('name', sorted(SHAPES))
@pytest.mark.parametrize('blocks', ['fixed', 'dynamic'])
def test_shapes(name, blocks):
    px = SHAPES[name]()
    _, kinds, _ = check_roundtrip(px, blocks=blocks)
    assert set(kinds) == {2 if blocks == 'dynamic' else 1}
    assert len(kinds) == -(-px.shape[0] * (1 + 3 * px.shape[1]) // SEG)


def test_fifteen_bit_codes():
    """One row of fibonacci_bytes.  With 14 values the block's histogram is 1 (end of block), 1 (the filter byte), 2, 3, 5, ...: 16 leaves whose Huffman
    code is 15 bits deep whatever the tie rule, exactly the limit, so the encoder sends it as it is and the kernel's symbol decode runs over all 15
    lengths.  With 16 values the unlimited code is 17 deep and the encoder's length-limited code is what is decoded; its longest code is printed (9 bits on an MI355X run: the halving loop flattens the counts well below the limit)."""
    vals = E.fibonacci_bytes(14)
    px = E.from_bytes(vals, len(vals) // 3)
    data, kinds, tokens = check_roundtrip(px, blocks='dynamic', filter=0)
    hist = np.bincount([t[1] for t in tokens[0]] + [256])
    lit = [n for n in E.deflate_blocks(E.idat(data))[0]['lit_lengths'] if n]
    assert all(t[0] == 'L' for t in tokens[0]) and sorted(hist[hist > 0].tolist())[:4] == [1, 1, 2, 3] and E.huffman_depth(hist) == 15
    assert len(lit) == 16 and sorted(lit) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15]     # the only complete code of depth 15 on 16 leaves
    vals = E.fibonacci_bytes(16)
    px = E.from_bytes(vals, len(vals) // 3)
    assert px.shape[0] == 1
    data, kinds, tokens = check_roundtrip(px, blocks='dynamic', filter=0)
    hist = np.bincount([t[1] for t in tokens[0]] + [256])                               # all literals: the block's histogram is 1, 1, 2, 3, 5, ...
    lit = [n for n in E.deflate_blocks(E.idat(data))[0]['lit_lengths'] if n]
    assert all(t[0] == 'L' for t in tokens[0]) and E.huffman_depth(hist) > 15           # an unlimited code does not fit: the encoder's length-limited one,
    print(f'[png inflate] 16 Fibonacci values: unlimited depth {E.huffman_depth(hist)}, the encoder\'s length-limited code is {max(lit)} bits deep')
    assert max(lit) <= 15 and sum(2.0 ** -n for n in lit) == 1.0 and len(lit) == 18     # complete


def test_all_literal_page_sends_two_dummy_distance_codes():
    px = E.noise(9, 7, seed=11)
    data, kinds, tokens = check_roundtrip(px, blocks='dynamic', filter=0)
    assert all(t[0] == 'L' for t in tokens[0])
    assert [n for n in E.deflate_blocks(E.idat(data))[0]['dist_lengths'] if n] == [1, 1]


def test_flat_page_resolves_in_many_rounds():
    """White rows: distance-1 runs of 258 and 2-row matches, each sub-block's first match reaching into the sub-block before it, so the chain of pending
    matches is as long as the segment has sub-blocks."""
    px = E.white(43, 1024)                                                              # 3 segments
    data, kinds, tokens = check_roundtrip(px, blocks='dynamic')
    assert len(kinds) == 3
    lens = [t[1] for t in tokens[0] if t[0] == 'M']
    assert max(lens) == 258 and {t[2] for t in tokens[0] if t[0] == 'M'} & {1} and len(data) < px.nbytes // 50
    check_roundtrip(E.flat_layout(120, 200), blocks='fixed')


def test_forced_stored_and_mixed_files():
    px = _half_noise(120, 200)
    _, kinds, _ = check_roundtrip(px, blocks='stored')
    assert set(kinds) == {0}
    _, kinds, _ = check_roundtrip(px, blocks='auto')                                    # noise above, flat below
    assert len(kinds) == 2 and (1 in kinds or 2 in kinds)
    # 110 rows of 601 noise bytes fill the first segment: it stays stored, the flat rest does not -- one file mixes stored and Huffman segments
    px = np.concatenate([E.noise(110, 200, seed=4), E.white(10, 200)], 0)
    _, kinds, _ = check_roundtrip(px, blocks='auto')
    assert kinds[0] == 0 and kinds[1] in (1, 2)


def test_several_files_and_two_sizes_in_one_call():
    pages = [E.photo(70, 90, seed=1), E.flat_layout(70, 90, seed=2), E.glyphs(70, 90, seed=3)]
    files = [_encode(p) for p in pages]
    out, status, raws = _decode(files)
    assert all(r.kind == 'packed' for r in raws) and status.tolist() == [0, 0, 0]
    assert torch.is_tensor(out) and tuple(out.shape) == (3, 70, 90, 3)
    for o, p in zip(out.cpu().numpy(), pages):
        assert np.array_equal(o, p)
    # two sizes, and a stored-block file of the first size: three groups, results in the order given
    other = E.photo(33, 47, seed=4)
    buf = io.BytesIO()
    import PIL.Image
    PIL.Image.fromarray(pages[1], 'RGB').save(buf, format='png', compress_level=0)
    out, status, raws = _decode([files[0], _encode(other), buf.getvalue(), files[2]])
    assert [r.kind for r in raws] == ['packed', 'packed', 'stored', 'packed'] and isinstance(out, list) and status.tolist() == [0, 0, 0]
    for o, p in zip(out, [pages[0], other, pages[1], pages[2]]):
        assert np.array_equal(o.cpu().numpy(), p)
    # a standalone call checks the status itself
    from layoutdetr_amd.training.dataset_layoutganpp import decode_pages
    assert np.array_equal(decode_pages(raws[:1], _dev())[0].cpu().numpy(), pages[0])


def test_index_false_writes_todays_file():
    from layoutdetr_amd import render
    for px, kw in ((E.photo(100, 300), {}), (_half_noise(120, 200), {}), (E.glyphs(40, 60), dict(blocks='fixed', filter=4))):
        grid = torch.from_numpy(px).to(_dev())
        plain = render.encode_png(grid, **kw).numpy().tobytes()
        E.check_file(plain, px)                                                         # IHDR, IDAT .., IEND only; every checksum; Pillow's pixels
        indexed = render.encode_png(grid, index=True, **kw).numpy().tobytes()
        n = struct.unpack('>I', indexed[33:37])[0]
        assert indexed[37:41] == b'ldIX' and indexed[:33] + indexed[33 + 12 + n:] == plain
        assert 12 + n <= render.png_index_bytes(*px.shape[:2]) < 12 + n + 16


def test_pin_memory_of_a_packed_page():
    from layoutdetr_amd.training.dataset_layoutganpp import decode_pages, scan_png
    px = E.glyphs(30, 40)
    data = _encode(px)
    raw = scan_png(data, packed=True)
    q = raw.pin_memory()
    assert q.kind == 'packed' and q.packed is raw.packed and q.tensor().is_pinned() and not raw.tensor().is_pinned() and bytes(q.tensor().numpy()) == data
    assert np.array_equal(decode_pages([q], _dev())[0].cpu().numpy(), px)


def test_save_png_with_index(tmp_path):
    from layoutdetr_amd import render
    from layoutdetr_amd.training.dataset_layoutganpp import scan_png
    px = E.flat_layout(50, 70)
    grid = torch.from_numpy(px).to(_dev())
    render.save_png(grid, str(tmp_path / 'a.png'), encoder='device', index=True)
    assert scan_png((tmp_path / 'a.png').read_bytes(), packed=True).kind == 'packed'
    with pytest.raises(ValueError, match='index'):
        render.save_png(grid, str(tmp_path / 'b.png'), encoder='pillow', index=True)


def test_packed_dataset_equals_device_mode(tmp_path):
    import os
    import PIL.Image
    from layoutdetr_amd import repack_dataset as R
    from layoutdetr_amd.training import dataset_layoutganpp as D
    tiny = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dataset_tiny.zip')
    dst = str(tmp_path / 'packed.zip')
    calls = []

    def recode(data, blocks):
        calls.append(blocks)
        if len(calls) == 2:                                                             # one page as a foreign file: Pillow's level 6
            buf = io.BytesIO()
            PIL.Image.open(io.BytesIO(data)).save(buf, format='png', compress_level=6)
            return buf.getvalue(), 'decoded'
        return R._device_recode(data, blocks)
    st = R.repack(tiny, dst, 'best', recode=recode)
    assert st['pages'] == 3
    with zipfile.ZipFile(tiny) as zin, zipfile.ZipFile(dst) as zout:
        assert zout.namelist() == zin.namelist()
        assert all(zout.read(n) == zin.read(n) for n in zin.namelist() if not R.is_page(n))
    ref, ds = D.LayoutDataset(tiny, mode='device'), D.LayoutDataset(dst, mode='packed')
    items = [ds[i] for i in range(len(ds))]
    assert ds.route_counts == {'raw': 0, 'packed': 2, 'decoded': 1}
    for i, (s, _) in enumerate(items):
        want = ref[i][0]
        page = s['background']
        if isinstance(page, D.RawPage):
            page = D.decode_pages([page], _dev())[0].cpu().numpy()
        assert page.dtype == np.uint8 and np.array_equal(page, want['background'])
        for k in ('bboxes', 'labels', 'mask'):
            assert np.array_equal(s[k], want[k])
    # the batch path: file bytes up, decoded and resized there; the status words are looked at one call later and at close()
    batch, _ = ds.collate(items)
    want, _ = ref.collate([ref[i] for i in range(len(ref))])
    got = D.batch_backgrounds_to_device(batch['background'], 64, _dev())
    assert len(D._pending_status) == 1
    assert torch.equal(got, D.batch_backgrounds_to_device(want['background'], 64, _dev()))
    assert D._pending_status == []
    D.batch_backgrounds_to_device(batch['background'], 64, _dev())
    ds.close()
    assert D._pending_status == []
    ref.close()
