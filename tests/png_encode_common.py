"""Shared by the device PNG encoder's tests (test_png_encode_cpu.py, test_png_encode_gpu.py): seeded image generators, a numpy restatement of the
row-filter rule, a chunk walker, decoders (Pillow, zlib) and a plain-Python deflate token reader that shows which block types, match lengths,
distances and code lengths a file holds.  Nothing here touches the GPU or the library."""
import io
import struct
import zlib

import numpy as np

import png_decode_common as P

SIGNATURE = b'\x89PNG\r\n\x1a\n'


# ---- images (uint8 [H, W, 3])

def noise(H, W, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


def white(H, W):
    return np.full((H, W, 3), 255, np.uint8)


def flat_layout(H, W, seed=1):
    """A white page with a dozen flat rectangles: what a `layouts` snapshot cell looks like."""
    rng = np.random.RandomState(seed)
    im = white(H, W)
    for _ in range(12):
        x0, y0 = rng.randint(0, max(W - 8, 1)), rng.randint(0, max(H - 8, 1))
        w, h = rng.randint(4, max(W // 2, 5)), rng.randint(4, max(H // 2, 5))
        im[y0:y0 + h, x0:x0 + w] = rng.randint(0, 256, 3)
    return im


def glyphs(H, W, seed=2):
    """Rows of 5 x 7 dot patterns from an alphabet of 16, mostly black on white: text-like content."""
    rng = np.random.RandomState(seed)
    im = white(H, W)
    alphabet = rng.rand(16, 7, 5) < 0.45
    for y in range(2, H - 9, 10):
        for x in range(2, W - 7, 7):
            col = (0, 0, 0) if rng.rand() < 0.8 else tuple(int(v) for v in rng.randint(0, 256, 3))
            im[y:y + 7, x:x + 5][alphabet[rng.randint(0, 16)]] = col
    return im


def photo(H, W, seed=3):
    """Smooth waves plus sensor-like noise: photo-like content."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(6):
            out[..., c] += rng.rand() * 40 * np.sin(xx * rng.rand() * 0.2 + yy * rng.rand() * 0.2 + rng.rand() * 6)
    out += 128 + rng.randn(H, W, 3) * 4
    return np.clip(out, 0, 255).astype(np.uint8)


def gradient(H, W):
    """Linear ramps: down the rows in R, along the row in G, diagonal in B."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(3 * yy) % 256, (2 * xx) % 256, (xx + 2 * yy) % 256], -1).astype(np.uint8)


def from_bytes(values, W):
    """A byte string laid out as the pixels of a W-wide image (zero padded): with filter 0 the stream's row payloads are these bytes."""
    values = np.asarray(values, np.uint8)
    H = max((len(values) + 3 * W - 1) // (3 * W), 1)
    a = np.zeros(H * W * 3, np.uint8)
    a[:len(values)] = values
    return a.reshape(H, W, 3)


def fibonacci_bytes(nsym=16, seed=3, distances=(1, 2, 3, 4, 6, 9, 12)):
    """nsym non-zero byte values with counts 2, 3, 5, 8, ... (the largest one raised until the total is a multiple of 3), ordered so that no three
    bytes repeat at any of `distances`: an encoder that looks only there finds no match.  As ONE row under filter 0 the block's histogram is then
    1 (end of block), 1 (the filter byte), 2, 3, 5, ...: Fibonacci, whose unlimited Huffman code is nsym + 1 bits deep whatever the tie rule."""
    fib = [2, 3]
    while len(fib) < nsym:
        fib.append(fib[-1] + fib[-2])
    fib[-1] += -sum(fib) % 3
    left = {(k * 11 + 3) % 256: c for k, c in enumerate(fib)}
    rng = np.random.RandomState(seed)
    s = []
    while any(left.values()):
        ok = [v for v, c in left.items() if c and not any(len(s) >= d + 2 and s[-d] == v and s[-1] == s[-1 - d] and s[-2] == s[-2 - d] for d in distances)]
        assert ok, 'no symbol fits: try another seed'
        ok.sort(key=lambda v: -left[v])
        v = ok[0] if rng.rand() < 0.7 or len(ok) == 1 else ok[rng.randint(1, len(ok))]      # mostly the most frequent one left, so the tail is not one symbol
        s.append(v)
        left[v] -= 1
    return np.array(s, np.uint8)


def huffman_depth(counts):
    """The longest code of an unlimited Huffman code of the non-zero counts."""
    import heapq
    heap = [(int(c), 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


# ---- the filter rule

def filter_choice(pixels):
    """(types [H], stream bytes): per row the filter with the minimum sum of absolute residuals, residuals read as signed bytes, ties to the lowest
    type; PNG's arithmetic (png_decode_common.filter_rows)."""
    H, W, _ = pixels.shape
    cand = np.stack([np.frombuffer(P.filter_rows(pixels, (k,)), np.uint8).reshape(H, 1 + 3 * W) for k in range(5)])
    cost = np.abs(cand[:, :, 1:].view(np.int8).astype(np.int64)).sum(-1)                # [5, H]
    types = np.argmin(cost, 0)                                                          # the first minimum: the lowest type
    stream = cand[types, np.arange(H)]
    return types, stream.tobytes()


# ---- files

def chunks(data):
    """[(type, payload, CRC field)] of a PNG file; asserts the signature and that the chunks tile the file."""
    data = bytes(data)
    assert data[:8] == SIGNATURE
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        out.append((data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n], struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0]))
        pos += 12 + n
    assert pos == len(data) and out[-1][0] == b'IEND'
    return out


def idat(data):
    return b''.join(d for t, d, _ in chunks(data) if t == b'IDAT')


def pillow_decode(data):
    import PIL.Image
    im = PIL.Image.open(io.BytesIO(bytes(data)))
    assert im.mode == 'RGB'
    return np.array(im)


def check_file(data, pixels):
    """The whole-file contract: every CRC, the zlib stream (length and Adler-32), Pillow's pixels.  Returns the filtered stream."""
    data = bytes(data)
    H, W, _ = pixels.shape
    ch = chunks(data)
    assert [t for t, _, _ in ch] == [b'IHDR'] + [b'IDAT'] * (len(ch) - 2) + [b'IEND']
    for t, d, crc in ch:
        assert crc == zlib.crc32(t + d), t
    assert ch[0][1] == struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)
    stream = zlib.decompress(idat(data))                                                # raises on a wrong Adler-32
    assert len(stream) == H * (1 + 3 * W)
    assert np.array_equal(pillow_decode(data), pixels)
    return stream


# ---- a deflate token reader

_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits(object):
    def __init__(self, data):
        self.d, self.p = data, 0

    def get(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << i
            self.p += 1
        return v


def _canonical(lengths):
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return table


def _symbol(br, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | br.get(1)
        if (n, code) in table:
            return table[(n, code)]
    raise ValueError('bad Huffman code')


def deflate_blocks(zdata):
    """The blocks of a zlib stream: [dict(type, final, n_stored | tokens, lit_lengths, dist_lengths)], tokens = ('L', byte) | ('M', length, distance)."""
    br = _Bits(bytes(zdata))
    br.get(16)
    out = []
    while True:
        final, btype = br.get(1), br.get(2)
        blk = dict(type=btype, final=final)
        if btype == 0:
            br.p = (br.p + 7) // 8 * 8
            n, nn = br.get(16), br.get(16)
            assert n ^ nn == 0xffff
            blk['n_stored'] = n
            br.p += 8 * n
        else:
            if btype == 1:
                lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dist = [5] * 32
            else:
                hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[_CLORDER[k]] = br.get(3)
                blk['cl_lengths'] = cl
                ct, lens = _canonical(cl), []
                while len(lens) < hlit + hdist:
                    s = _symbol(br, ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + br.get(2))
                    elif s == 17:
                        lens += [0] * (3 + br.get(3))
                    else:
                        lens += [0] * (11 + br.get(7))
                lit, dist = lens[:hlit], lens[hlit:]
            blk['lit_lengths'], blk['dist_lengths'] = lit, dist
            lt, dt, toks = _canonical(lit), _canonical(dist), []
            while True:
                s = _symbol(br, lt)
                if s == 256:
                    break
                if s < 256:
                    toks.append(('L', s))
                else:
                    n = _LBASE[s - 257] + br.get(_LEXT[s - 257])
                    d = _symbol(br, dt)
                    toks.append(('M', n, _DBASE[d] + br.get(_DEXT[d])))
            blk['tokens'] = toks
        out.append(blk)
        if final:
            return out
