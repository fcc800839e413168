"""Indexed page PNGs, the part that needs no GPU: ldetr_png_scan_packed against the plain-Python restatement of the format
(png_inflate_common), the Python surface around it, the repack tool with the encoder stubbed by the restatement, the ABI bookkeeping, and the inflate
kernel's own source built for the host with the sanitizers (tools/png_inflate_hostcheck.cpp), which is where corrupted files go -- never to a GPU."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import zipfile

import numpy as np
import pytest
import torch

import png_decode_common as P
import png_encode_common as E
import png_inflate_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, 'tests', 'golden', 'dataset_tiny.zip')


def _half_noise(H, W):
    return np.concatenate([E.noise(H // 2, W, seed=4), E.flat_layout(H - H // 2, W, seed=5)], 0)


# name -> (pixels, block type per segment): one short sub-block; two segments with the seam mid-row; stored and compressed segments in one file;
# 15-bit codes; no match at all (two dummy distance codes); long chains of matches across sub-blocks
CASES = {
    '1x1_fixed': lambda: (E.noise(1, 1), 'fixed'),
    '3x5_dynamic': lambda: (E.noise(5, 3), 'dynamic'),
    '300x100_flat_dynamic': lambda: (E.flat_layout(100, 300), 'dynamic'),
    '300x100_photo_fixed_dynamic': lambda: (E.photo(100, 300), ('fixed', 'dynamic')),
    '200x120_stored_dynamic': lambda: (_half_noise(120, 200), ('stored', 'dynamic')),
    'fibonacci_row': lambda: (E.from_bytes(E.fibonacci_bytes(14), len(E.fibonacci_bytes(14)) // 3), 'dynamic', dict(schedule=(0,))),
    'white_1024x40': lambda: (E.white(40, 1024), 'dynamic'),
}
_cache = {}


def packed(name):
    if name not in _cache:
        px, kinds, *kw = CASES[name]()
        _cache[name] = (px, C.write_packed_png(px, kinds, **(kw[0] if kw else {})))
    return _cache[name]


@pytest.fixture(scope='module')
def hostcheck(tmp_path_factory):
    """The inflate kernel's source compiled for the host with AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program.  The sanitizer
    runtimes are linked statically, so the program runs in whatever environment the tests run in and needs nothing preloaded."""
    exe = str(tmp_path_factory.mktemp('hostcheck') / 'png_inflate_hostcheck')
    flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    tried = []
    for cxx, static in (('g++', ['-static-libasan', '-static-libubsan']), ('clang++', ['-static-libsan'])):      # (clang's runtimes are static by default)
        if shutil.which(cxx):
            r = subprocess.run([cxx] + flags + static + ['-o', exe, os.path.join(ROOT, 'tools', 'png_inflate_hostcheck.cpp')], capture_output=True, text=True)
            if r.returncode == 0:
                break
            tried.append(f'{cxx}: {r.stderr[-500:]}')
    else:
        raise AssertionError('no host C++ compiler links the sanitizers statically: ' + ' | '.join(tried))

    def run(data, table, index_off, H, W, stream, tmp=os.path.dirname(exe)):
        job = os.path.join(tmp, 'job.bin')
        with open(job, 'wb') as f:
            f.write(C.hostcheck_job(data, table, index_off, H, W, stream))
        r = subprocess.run([exe, job], capture_output=True, text=True)
        assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-2000:]
        assert r.returncode in (0, 3, 4), (r.returncode, r.stdout, r.stderr[-2000:])
        return r.returncode, int(r.stdout.split()[1])
    return run


def test_cases_hold_what_they_are_named_for():
    blk = E.deflate_blocks(E.idat(packed('fibonacci_row')[1].data))[0]
    assert max(blk['lit_lengths']) == 15 and all(t[0] == 'L' for t in blk['tokens'])                 # codes of the full 15 bits
    blk = E.deflate_blocks(E.idat(packed('3x5_dynamic')[1].data))[0]
    assert [n for n in blk['dist_lengths'] if n] == [1, 1] and all(t[0] == 'L' for t in blk['tokens'])       # no match: two dummy distance codes
    f = packed('white_1024x40')[1]
    first = [toks[0] for toks in f.tokens[0][1:]]
    assert len(first) == 127 and sum(1 for t in first if t[0] == 'M' and t[2] == 1) > 100           # sub-blocks start with a match into the one before: a long chain of rounds
    assert [k for _, _, k, _ in packed('200x120_stored_dynamic')[1].table] == [0, 2]


# ---- the host scan

@pytest.mark.parametrize('name', sorted(CASES))
def test_scan_equals_the_restatement(name):
    from layoutdetr_amd.training.dataset_layoutganpp import RawPage, scan_png
    px, f = packed(name)
    assert scan_png(f.data) is None                                                     # the stored scan alone does not take it
    raw = scan_png(f.data, packed=True, verify=True)
    assert isinstance(raw, RawPage) and raw.kind == 'packed' and raw.segments is None
    assert (raw.height, raw.width) == px.shape[:2] and raw.shape == px.shape
    seg, index_off = raw.packed
    assert seg.dtype == np.int64 and seg.tolist() == [list(r) for r in f.table]
    assert index_off == f.index_off
    assert raw.row_starts.dtype == np.int32 and raw.row_starts.tolist() == f.row_starts
    assert bytes(raw.data) == f.data


def test_row_starts_follow_the_index_filter_bytes():
    bars = np.repeat(E.noise(130, 1, seed=6), 20, axis=1)                               # every row one colour: Sub leaves two non-zero bytes, Up a whole row
    px = np.concatenate([E.photo(70, 20, seed=9), bars], 0)
    f = C.write_packed_png(px, 'fixed')
    assert len(f.row_starts) > 1 and len(set(f.types.tolist())) > 1
    from layoutdetr_amd.training.dataset_layoutganpp import scan_png
    assert scan_png(f.data, packed=True).row_starts.tolist() == f.row_starts


def test_stored_files_stay_stored_and_foreign_files_are_not_eligible():
    import PIL.Image
    from layoutdetr_amd.training.dataset_layoutganpp import scan_png
    px = E.photo(40, 50)
    buf = io.BytesIO()
    PIL.Image.fromarray(px, 'RGB').save(buf, format='png', compress_level=0)
    a, b = scan_png(buf.getvalue()), scan_png(buf.getvalue(), packed=True)
    assert a.kind == b.kind == 'stored' and b.packed is None
    assert np.array_equal(a.segments, b.segments) and np.array_equal(a.row_starts, b.row_starts) and (a.width, a.height) == (b.width, b.height) and bytes(a.data) == bytes(b.data)
    buf = io.BytesIO()
    PIL.Image.fromarray(px, 'RGB').save(buf, format='png', compress_level=6)
    assert scan_png(buf.getvalue(), packed=True) is None and scan_png(buf.getvalue()) is None
    # an indexed file whose segments are all stored is a stored-block file: the stored scan takes it, the index is not needed
    f = C.write_packed_png(px, 'stored')
    assert scan_png(f.data, packed=True).kind == 'stored'
    # a wrong version, another segment size: well-formed, not this library's
    px, f = packed('300x100_flat_dynamic')
    for kw in (dict(version=2), dict(seg=32768), dict(sub=256)):
        assert scan_png(C.replace_index(f, C.index_payload(f.types, f.entries, **kw)), packed=True) is None
    # the index behind the first IDAT, no index at all
    ch = E.chunks(f.data)
    moved = E.SIGNATURE + b''.join(P.chunk(t, d) for t, d, _ in [ch[0], ch[2], ch[1]] + ch[3:])
    assert scan_png(moved, packed=True) is None
    assert scan_png(E.SIGNATURE + b''.join(P.chunk(t, d) for t, d, _ in ch if t != b'ldIX'), packed=True) is None


def test_scan_refuses_a_broken_index():
    from layoutdetr_amd.training.dataset_layoutganpp import scan_png
    px, f = packed('300x100_flat_dynamic')
    good = C.index_payload(f.types, f.entries)
    assert scan_png(C.replace_index(f, good), packed=True) is not None

    def entries(fn):
        es = [list(e) for e in f.entries]
        fn(es)
        return C.replace_index(f, C.index_payload(f.types, es))
    nbits = 8 * f.table[1][1]
    cases = {
        'does not lie behind': entries(lambda es: es[0].__setitem__(7, es[0][6])),                  # not strictly increasing
        'outside the chunk': entries(lambda es: es[1].__setitem__(len(es[1]) - 1, nbits + 5)),      # past the chunk
        'block header ends': entries(lambda es: es[1].__setitem__(0, es[1][0] - 8)),                # into the trees
        'truncated ldIX': C.replace_index(f, good[:8]),
        'ldIX chunk of': C.replace_index(f, good[:-4]),
        'filter byte 5': C.replace_index(f, C.index_payload([5] + list(f.types[1:]), f.entries)),
    }
    for match, data in cases.items():
        with pytest.raises(ValueError, match=match):
            scan_png(data, packed=True)
    with pytest.raises(ValueError, match='truncated file'):
        scan_png(f.data[:-7], packed=True)
    # the raw entry's capacity protocol: a table that is given and too small is an argument error
    from layoutdetr_amd import _lib
    lib = _lib.load()
    arr = np.frombuffer(f.data, np.uint8)
    w, h, k, r, ix = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    seg = np.zeros((1, 4), np.int64)
    rc = lib.ldetr_png_scan_packed(arr.ctypes.data, arr.size, ctypes.byref(w), ctypes.byref(h), seg.ctypes.data, 1, ctypes.byref(k), ctypes.byref(ix), None, 0, ctypes.byref(r))
    assert rc == 1 and k.value == 2 and 'segment table too small' in lib.ldetr_last_error().decode()
    rc = lib.ldetr_png_scan_packed(arr.ctypes.data, arr.size, ctypes.byref(w), ctypes.byref(h), None, 0, ctypes.byref(k), ctypes.byref(ix), None, 0, ctypes.byref(r))
    assert rc == 0 and (w.value, h.value, k.value, r.value, ix.value) == (300, 100, 2, len(f.row_starts), f.index_off)


# ---- the Python surface

def test_raw_page_keeps_its_five_argument_constructor():
    from layoutdetr_amd.training.dataset_layoutganpp import RawPage
    p = RawPage(np.zeros(4, np.uint8), 2, 3, np.zeros((1, 3), np.int64), np.zeros(1, np.int32))
    assert p.kind == 'stored' and p.packed is None and p.shape == (3, 2, 3)
    assert RawPage.__slots__ == ('data', 'width', 'height', 'segments', 'row_starts', 'kind', 'packed')
    with pytest.raises(ValueError, match='packed'):
        RawPage(np.zeros(4, np.uint8), 2, 3, None, np.zeros(1, np.int32), 'packed')
    with pytest.raises(AttributeError):
        p.other = 1


def test_pin_memory_keeps_the_packed_fields(monkeypatch):
    """What DataLoader(pin_memory=True) calls.  Page-locked memory itself needs the GPU runtime (test_png_inflate_gpu.py pins for real): here the tensor's
    pin_memory is replaced by a copy, and the RawPage around it must come back whole."""
    from layoutdetr_amd.training.dataset_layoutganpp import scan_png
    px, f = packed('3x5_dynamic')
    raw = scan_png(f.data, packed=True)
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self, device=None: self.clone())
    q = raw.pin_memory()
    assert q is not raw and q.kind == 'packed' and q.packed is raw.packed and q.row_starts is raw.row_starts and q.segments is None
    assert (q.width, q.height) == (raw.width, raw.height) and torch.is_tensor(q.data) and q.data.data_ptr() != raw.tensor().data_ptr() and bytes(q.data.numpy()) == f.data


def test_dataset_mode_switches(monkeypatch):
    from layoutdetr_amd import dropin
    from layoutdetr_amd.training import dataset_layoutganpp as D
    assert D.DATASET_MODES == ('device', 'raw', 'packed', 'reference')
    env = {}
    assert dropin.parse_options(['--dataset-mode=packed', 'train.py', '--gpus=1'], env) == ['train.py', '--gpus=1']
    assert env == {'LDETR_DATASET_MODE': 'packed'}
    with pytest.raises(SystemExit, match='packed'):
        dropin.parse_options(['--dataset-mode=host', 'train.py'], {})
    monkeypatch.setenv('LDETR_DATASET_MODE', 'packed')
    assert D.default_dataset_mode() == 'packed'
    ds = D.LayoutDataset(TINY)
    assert ds.mode == 'packed' and ds.route_counts == {'raw': 0, 'packed': 0, 'decoded': 0}
    ds.close()
    monkeypatch.delenv('LDETR_DATASET_MODE')
    assert D.default_dataset_mode() == 'device'
    ds = D.LayoutDataset(TINY, mode='raw')
    assert ds.route_counts == {'raw': 0, 'decoded': 0}
    ds.close()
    with pytest.raises(ValueError, match='packed'):
        D.LayoutDataset(TINY, mode='indexed')


def test_packed_mode_items_without_a_gpu(tmp_path):
    """mode='packed' on an archive repacked by the restatement: indexed pages leave as file bytes, a Pillow level-6 page is decoded on the host."""
    import PIL.Image
    from layoutdetr_amd import repack_dataset as R
    from layoutdetr_amd.training import dataset_layoutganpp as D
    dst = str(tmp_path / 'packed.zip')

    def recode(data, blocks):
        px = np.array(PIL.Image.open(io.BytesIO(data)))
        if recode.n == 0:                                                               # one page as a foreign compressed file
            buf = io.BytesIO()
            PIL.Image.fromarray(px, 'RGB').save(buf, format='png', compress_level=6)
            new = buf.getvalue()
        else:
            new = C.write_packed_png(px, 'fixed' if blocks == 'best' else 'stored').data
        recode.n += 1
        return new, 'decoded'
    recode.n = 0
    st = R.repack(TINY, dst, 'best', recode=recode)
    assert st['pages'] == recode.n >= 2 and st['routes'] == {'raw': 0, 'decoded': st['pages']} and st['bytes_before'] > 0 and st['bytes_after'] > 0
    ref, ds = D.LayoutDataset(TINY, mode='device'), D.LayoutDataset(dst, mode='packed')
    for i in range(len(ds)):
        a, b = ds[i][0]['background'], ref[i][0]['background']
        if isinstance(a, D.RawPage):
            assert a.kind == 'packed' and a.shape == b.shape and np.array_equal(E.pillow_decode(bytes(a.data)), b)
        else:
            assert np.array_equal(a, b)
    assert ds.route_counts == {'raw': 0, 'packed': st['pages'] - 1, 'decoded': 1}
    ds.close()
    ref.close()


def test_repack_arguments_and_entry_selection(tmp_path):
    from layoutdetr_amd import repack_dataset as R
    a = R.parse_args(['a.zip', 'b.zip'])
    assert (a.src, a.dst, a.blocks) == ('a.zip', 'b.zip', 'best')
    assert R.parse_args(['a.zip', 'b.zip', '--blocks', 'stored']).blocks == 'stored' and R.BLOCKS == {'best': 'auto', 'stored': 'stored'}
    for bad in (['a.zip'], ['a.zip', 'a.zip'], ['a.zip', 'b.zip', '--blocks=fixed']):
        with pytest.raises(SystemExit):
            R.parse_args(bad)
    assert R.is_page('x/y_background_orig.png') and not R.is_page('x/y_0_patch_orig.png') and not R.is_page('non_image.json')
    import PIL.Image
    seen = []

    def recode(data, blocks):
        seen.append(blocks)
        return C.write_packed_png(np.array(PIL.Image.open(io.BytesIO(data))), 'dynamic').data, 'raw'
    dst = str(tmp_path / 'out.zip')
    st = R.repack(TINY, dst, 'stored', recode=recode)
    with zipfile.ZipFile(TINY) as zin, zipfile.ZipFile(dst) as zout:
        assert zout.namelist() == zin.namelist()
        pages = [n for n in zin.namelist() if n.endswith('_background_orig.png')]
        assert len(pages) == st['pages'] == len(seen) > 0 and set(seen) == {'stored'} and st['routes'] == {'raw': len(pages), 'decoded': 0}
        for n in zin.namelist():
            if n in pages:
                assert zout.getinfo(n).compress_type == zipfile.ZIP_STORED
                assert np.array_equal(E.pillow_decode(zout.read(n)), E.pillow_decode(zin.read(n)))
                assert [t for t, _, _ in E.chunks(zout.read(n))][1] == b'ldIX'
            else:
                assert zout.read(n) == zin.read(n) and zout.getinfo(n).compress_type == zin.getinfo(n).compress_type
        assert st['bytes_before'] == sum(zin.getinfo(n).file_size for n in pages) and st['bytes_after'] == sum(zout.getinfo(n).file_size for n in pages)


def test_header_mirror_and_abi_version():
    from layoutdetr_amd import _lib, render
    header = open(os.path.join(ROOT, 'include', 'ldetr_hip.h')).read()
    for name in ('ldetr_png_index_bytes', 'ldetr_png_scan_packed', 'ldetr_png_inflate_u8'):
        assert name in _lib.SIGNATURES and f'int {name}(' in header and header[:header.index('#ifndef LDETR_HIP_H')].count(name) == 1
    lib = _lib.load()
    assert _lib.ABI_VERSION == 25 and lib.ldetr_abi_version() == 25
    sizes = (ctypes.c_int32 * 8)(*([-1] * 8))
    lib.ldetr_struct_sizes(sizes)
    assert list(sizes)[6:] == [-1, -1]
    assert ctypes.sizeof(_lib.PngInflateArgs) == 24 + 15 * 8 and ctypes.sizeof(_lib.PngEncodeArgs) == 24 + 8 * 8
    fields = [f for f, _ in _lib.PngInflateArgs._fields_]
    decl = header[header.index('typedef struct ldetr_png_inflate_args {'):header.index('} ldetr_png_inflate_args;')]
    at = [decl.index(f' {f};') if f' {f};' in decl else decl.index(f' {f},') if f' {f},' in decl else decl.index(f', {f};') for f in fields]
    assert at == sorted(at)
    for bit, name in ((1, 'CODE'), (2, 'COUNT'), (4, 'HEADER'), (8, 'DISTANCE'), (16, 'TRAILER'), (32, 'FILTER'), (64, 'STUCK'), (128, 'TABLE')):
        assert f'#define LDETR_PNG_INFLATE_{name} {bit} ' in header
    # the index adds its chunk, rounded up to 16: 12 bytes of framing, 12 of header, H filter bytes, 4 per sub-block
    for H, W in ((1, 1), (100, 300), (1024, 1024), (21, 1025)):
        nsub = sum(-(-(b - a) // 512) for a, b in render.png_encode_segments(H, W))
        assert render.png_index_bytes(H, W) == -(-(12 + 12 + H + 4 * nsub) // 16) * 16
    with pytest.raises(ValueError, match='16384'):
        render.png_index_bytes(0, 4)
    # a block of the wrong size or with a reserved bit is refused before any GPU work
    a = _lib.PngInflateArgs(struct_bytes=8)
    assert lib.ldetr_png_inflate_u8(ctypes.byref(a), None) == 1 and 'argument block' in lib.ldetr_last_error().decode()


# ---- the kernel's source on the host, under the sanitizers

@pytest.mark.parametrize('name', sorted(CASES))
def test_host_build_reproduces_the_stream(hostcheck, name):
    px, f = packed(name)
    H, W, _ = px.shape
    assert hostcheck(f.data, f.table, f.index_off, H, W, f.stream) == (0, 0)


def _token_bit(f, segment, want, end=False):
    """(bit offset in the segment's chunk, token) of the first token `want` accepts, by walking the restatement's own bits (fixed codes); end=True: the
    bit offset behind the segment's last token instead."""
    lit = C.FIXED_LIT
    lc = {s: n for s, n in enumerate(lit)}
    for k, toks in enumerate(f.tokens[segment]):
        bit = f.entries[segment][k]
        for t in toks:
            if want(t):
                return bit, t
            if t[0] == 'L':
                bit += lc[t[1]]
            else:
                s, eb, _ = C._len_symbol(t[1])
                bit += lc[s] + eb + 5 + C._dist_symbol(t[2])[1]
    if end:
        return bit
    raise AssertionError('no such token')


def test_host_build_flags_corrupted_files(hostcheck):
    """Each corruption gives a non-zero status and no sanitizer report; none of these files ever goes to a GPU."""
    px, f = packed('300x100_flat_dynamic')
    H, W, _ = px.shape
    run = lambda data, stream=f.stream: hostcheck(data, f.table, f.index_off, H, W, stream)
    assert run(f.data) == (0, 0)
    e = f.entries
    # an index entry moved by one bit
    rc, status = run(C.set_entry(f.data, f, 0, 5, e[0][5] + 1))
    assert rc == 3 and status != 0
    rc, status = run(C.set_entry(f.data, f, 1, 3, e[1][3] - 1))
    assert rc == 3 and status != 0
    # entry 0 pointing into the trees: the header check
    rc, status = run(C.set_entry(f.data, f, 1, 0, e[1][0] - 40))
    assert rc == 3 and status & 4
    # a stream filter byte that differs from the index
    at = f.index_off + 12 + 7
    rc, status = run(f.data[:at] + bytes([(f.data[at] + 1) % 5]) + f.data[at + 1:])
    assert (rc, status) == (3, 32)
    # an entry far outside the chunk, a chunk cut short in the table, garbage where the tokens were: errors, not faults
    rc, status = run(C.set_entry(f.data, f, 0, 9, 0xfffffff0))
    assert rc == 3
    off, n = f.table[0][:2]
    noise = np.random.RandomState(0).randint(0, 256, n - 64, dtype=np.uint8).tobytes()
    rc, status = run(f.data[:off + 64] + noise + f.data[off + n:])
    assert rc == 3 and status != 0
    # with fixed codes the bits of single tokens are easy to reach
    px = E.flat_layout(60, 200, seed=8)
    g = C.write_packed_png(px, 'fixed')
    H, W, _ = px.shape
    base = 8 * g.table[0][0]
    bits = np.unpackbits(np.frombuffer(g.data, np.uint8), bitorder='little').copy()
    assert hostcheck(g.data, g.table, g.index_off, H, W, g.stream) == (0, 0)
    # a distance before the segment start: the first match of sub-block 0 sent with the 5-bit code of distance symbol 29 and all 13 extra bits set
    bit, t = _token_bit(g, 0, lambda t: t[0] == 'M')
    s, eb, _ = C._len_symbol(t[1])
    d0 = base + bit + C.FIXED_LIT[s] + eb
    far = bits.copy()
    far[d0:d0 + 5] = [1, 1, 1, 0, 1]                                                    # 29, top bit first
    rc, status = hostcheck(np.packbits(far, bitorder='little').tobytes(), g.table, g.index_off, H, W, g.stream)
    assert rc == 3 and status & 8
    # a missing end-of-block: code 256 (seven zero bits behind the last token) with its last bit set is code 257, a length.  Every token before it is
    # intact and the last sub-block still yields its bytes, so the trailer check is the only one that can fire
    at = _token_bit(g, 0, lambda t: False, end=True)
    assert not bits[base + at:base + at + 7].any() and bits[base + at + 7] == 1         # 256, then BFINAL = 1 of the empty stored block
    eob = bits.copy()
    eob[base + at + 6] = 1
    rc, status = hostcheck(np.packbits(eob, bitorder='little').tobytes(), g.table, g.index_off, H, W, g.stream)
    assert (rc, status) == (3, 16)
    # the empty stored block's LEN / NLEN overwritten
    tr = bytearray(g.data)
    tr[g.table[0][0] + g.table[0][1] - 8] = 1
    rc, status = hostcheck(bytes(tr), g.table, g.index_off, H, W, g.stream)
    assert (rc, status) == (3, 16)
