"""Shared by the stored-PNG decode tests (test_png_decode_cpu.py, test_png_decode_gpu.py): a small PNG writer that emits what the reference's
dataset_tool.py:325-363 makes Pillow emit (8-bit RGB, a zlib stream of stored blocks) with every degree of freedom the decoder must cope with
under the caller's control -- the filter of every row, the size of every stored block, the size of every IDAT chunk, ancillary chunks -- plus a
plain-Python walk of such a file (what `ldetr_png_scan` must return) and the case lists.  Expected pixels always come from Pillow."""
import io
import itertools
import struct
import zlib

import numpy as np


def filter_rows(pixels, schedule):
    """uint8 [H, W, 3] -> the filtered scanline stream, bytes of H * (1 + 3 W), row y filtered with schedule[y % len(schedule)]."""
    H, W, _ = pixels.shape
    rows = pixels.reshape(H, 3 * W).astype(np.int32)
    out = np.zeros((H, 1 + 3 * W), np.uint8)
    zero = np.zeros(3 * W, np.int32)
    for y in range(H):
        ft = int(schedule[y % len(schedule)])
        cur, up = rows[y], (rows[y - 1] if y else zero)
        a = np.concatenate([np.zeros(3, np.int32), cur[:-3]])
        c = np.concatenate([np.zeros(3, np.int32), up[:-3]])
        if ft == 0:
            pred = zero
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (a + up) >> 1
        elif ft == 4:
            p = a + up - c
            pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        else:
            pred = zero                                   # an invalid filter byte (the malformed cases): the bytes do not matter
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 0xff
    return out.tobytes()


def stored_zlib(stream, block_sizes):
    """A zlib stream of stored blocks only: block sizes cycle through `block_sizes` (0 allowed) until the payload is used up."""
    out = [b'\x78\x01']
    pos, n = 0, len(stream)
    sizes = itertools.cycle(block_sizes)
    if all(s == 0 for s in block_sizes):
        raise ValueError('block_sizes needs a non-zero entry')
    while True:
        size = min(next(sizes), 65535, n - pos)
        final = pos + size >= n
        out.append(struct.pack('<BHH', 1 if final else 0, size, size ^ 0xffff))
        out.append(stream[pos:pos + size])
        pos += size
        if final:
            break
    out.append(struct.pack('>I', zlib.adler32(stream)))
    return b''.join(out)


def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def png_file(W, H, zdata, chunk_sizes, before=(), after=(), depth=8, ctype=2, interlace=0, iend=True):
    out = [b'\x89PNG\r\n\x1a\n', chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, depth, ctype, 0, 0, interlace))]
    out += [chunk(k, d) for k, d in before]
    pos = 0
    sizes = itertools.cycle(chunk_sizes)
    while pos < len(zdata):
        size = next(sizes)
        out.append(chunk(b'IDAT', zdata[pos:pos + size]))
        pos += size
    out += [chunk(k, d) for k, d in after]
    if iend:
        out.append(chunk(b'IEND', b''))
    return b''.join(out)


def write_stored_png(pixels, schedule=(0,), block_sizes=(65535,), chunk_sizes=(1 << 30,), before=(), after=()):
    """uint8 [H, W, 3] -> PNG file bytes."""
    H, W, _ = pixels.shape
    return png_file(W, H, stored_zlib(filter_rows(pixels, schedule), block_sizes), chunk_sizes, before, after)


def pillow_decode(data):
    import PIL.Image
    return np.array(PIL.Image.open(io.BytesIO(data)))


def python_walk(data):
    """The segment table of a stored-block PNG by a plain-Python walk: [(offset in file, offset in stream, length)], one per contiguous payload run."""
    pos, idat = 8, []                                     # [(file offset of byte, ...)] via runs
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        if kind == b'IDAT':
            idat.append((pos + 8, n))
        if kind == b'IEND':
            break
        pos += 12 + n
    where = np.concatenate([np.arange(o, o + n, dtype=np.int64) for o, n in idat]) if idat else np.zeros(0, np.int64)      # logical zlib byte -> file offset
    z = bytes(data[i] for i in where) if len(where) < 4096 else np.frombuffer(data, np.uint8)[where].tobytes()
    segs, zp, sp = [], 2, 0
    while True:
        final, size, nsize = struct.unpack('<BHH', z[zp:zp + 5])
        assert (final >> 1) == 0 and size ^ nsize == 0xffff
        zp += 5
        lo = zp
        while lo < zp + size:                             # cut at file discontinuities
            hi = lo + 1
            while hi < zp + size and where[hi] == where[hi - 1] + 1:
                hi += 1
            segs.append((int(where[lo]), sp, hi - lo))
            sp += hi - lo
            lo = hi
        zp += size
        if final & 1:
            break
    return segs


# ---- the case lists

SIZES = [(1, 1), (1, 5), (2, 3), (7, 7), (80, 56), (63, 64), (65, 65), (40, 130), (1366, 3), (257, 129)]      # (W, H)

ANCILLARY_BEFORE = ((b'gAMA', struct.pack('>I', 45455)), (b'tEXt', b'Comment\x00stored-block test page'))
ANCILLARY_AFTER = ((b'tIME', struct.pack('>HBBBBB', 2024, 1, 2, 3, 4, 5)),)

LAYOUTS = {
    'one_block_one_chunk': dict(block_sizes=(65535,), chunk_sizes=(1 << 30,)),      # (a page above 65 535 stream bytes needs more blocks: the format's limit)
    'pillow_65535_65536': dict(block_sizes=(65535,), chunk_sizes=(65536,)),
    'blocks_1_chunks_3': dict(block_sizes=(1,), chunk_sizes=(3,)),
    'blocks_0_5_1_0_17_chunks_1_2_7_4': dict(block_sizes=(0, 5, 1, 0, 17), chunk_sizes=(1, 2, 7, 4)),
    'ancillary': dict(block_sizes=(65535,), chunk_sizes=(1 << 30,), before=ANCILLARY_BEFORE, after=ANCILLARY_AFTER),
}


def schedules(H, seed):
    """name -> per-row filter schedule: all-0 .. all-4, each filter type on row 0 with another type below it, a random mix."""
    out = {f'all_{f}': (f,) for f in range(5)}
    for f in range(5):
        out[f'row0_{f}_then_{(f + 2) % 5}'] = (f,) + ((f + 2) % 5,) * max(H - 1, 1)
    out['random_mix'] = tuple(int(v) for v in np.random.RandomState(seed).randint(0, 5, size=max(H, 1)))
    return out


SCHEDULE_NAMES = list(schedules(1, 0))


def noise_page(W, H, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


def case_files(W, H, schedule_name, seed=0):
    """One noise page of the size, filtered with the named schedule, written in every layout: (pixels, {layout: file bytes})."""
    px = noise_page(W, H, seed * 7919 + W * 131 + H)
    sched = schedules(H, seed + W + H)[schedule_name]
    return px, {name: write_stored_png(px, sched, **kw) for name, kw in LAYOUTS.items()}
