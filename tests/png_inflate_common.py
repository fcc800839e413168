"""Shared by the indexed-PNG inflate tests (test_png_inflate_cpu.py, test_png_inflate_gpu.py): a plain-Python restatement of the FILE FORMAT of DESIGN.md
section 18 -- not of the kernel.  Pixels and a block type per segment become tokens under the sub-block rule (64 KiB segments that no match crosses,
512-byte sub-blocks that no token crosses), the tokens become bits, and the bit offset of every sub-block's first token goes into the ldIX chunk.  The
deflate tables and the canonical-code rule are png_encode_common's.  Every file written here is checked with Pillow (pixels equal, the unknown chunk
ignored) and zlib (the joined IDAT inflates to the filtered stream), so the CPU tests need no file written by a GPU."""
import heapq
import struct
import zlib

import numpy as np

import png_decode_common as P
import png_encode_common as E

SEG, SUB = 65536, 512
KINDS = {'stored': 0, 'fixed': 1, 'dynamic': 2}
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def segments(total):
    return [(a, min(a + SEG, total)) for a in range(0, total, SEG)]


def tokenize(seg, distances):
    """One segment's bytes -> [tokens of sub-block 0, tokens of sub-block 1, ...], tokens = ('L', byte) | ('M', length, distance): greedy, the longest match
    of 3 .. 258 bytes among `distances` that ends inside the sub-block and starts inside the segment; ties to the first distance listed."""
    a = np.frombuffer(seg, np.uint8)
    n, out = len(a), []
    for start in range(0, n, SUB):
        end, i, toks = min(start + SUB, n), start, []
        while i < end:
            best, bd, maxlen = 0, 0, min(end - i, 258)
            if maxlen >= 3:
                for d in distances:
                    if d > i or not (a[i - d] == a[i] and a[i - d + 1] == a[i + 1] and a[i - d + 2] == a[i + 2]):
                        continue
                    if d >= maxlen:
                        neq = np.nonzero(a[i - d:i - d + maxlen] != a[i:i + maxlen])[0]
                        m = int(neq[0]) if len(neq) else maxlen
                    else:                                         # the match overlaps what it produces: byte by byte
                        m = 3
                        while m < maxlen and a[i - d + m] == a[i + m]:
                            m += 1
                    if m > best:
                        best, bd = m, d
            if best >= 3:
                toks.append(('M', best, bd))
                i += best
            else:
                toks.append(('L', int(a[i])))
                i += 1
        out.append(toks)
    return out


def _len_symbol(n):
    s = max(k for k in range(29) if E._LBASE[k] <= n)
    return 257 + s, E._LEXT[s], n - E._LBASE[s]


def _dist_symbol(d):
    s = max(k for k in range(30) if E._DBASE[k] <= d)
    return s, E._DEXT[s], d - E._DBASE[s]


def code_lengths(freq, limit=15):
    """Huffman code lengths of the non-zero frequencies (at least two of them), none longer than `limit`: frequencies are halved (rounding up) until
    the unlimited code fits."""
    freq = list(freq)
    while True:
        heap = [(f, s, (s,)) for s, f in enumerate(freq) if f]
        assert len(heap) >= 2
        heapq.heapify(heap)
        depth = [0] * len(freq)
        while len(heap) > 1:
            (fa, ka, sa), (fb, kb, sb) = heapq.heappop(heap), heapq.heappop(heap)
            for s in sa + sb:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, min(ka, kb), sa + sb))
        if max(depth) <= limit:
            return depth
        freq = [(f + 1) // 2 for f in freq]


def _codes(lengths):
    """symbol -> (length, code), the code's first bit being its top bit."""
    return {s: nc for nc, s in E._canonical(list(lengths)).items()}


class BitWriter(object):
    def __init__(self):
        self.bits = []

    def put(self, value, n):                                      # LSB first: header fields and extra bits
        self.bits += [(value >> k) & 1 for k in range(n)]

    def code(self, nc):                                           # a Huffman code: top bit first
        n, c = nc
        self.bits += [(c >> (n - 1 - k)) & 1 for k in range(n)]

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def tobytes(self):
        assert len(self.bits) % 8 == 0
        return np.packbits(np.array(self.bits, np.uint8), bitorder='little').tobytes()


def deflate_segment(seg, kind, last, zlib_header, distances):
    """-> (the bytes of the segment's IDAT chunk without the Adler-32, the index entries of its sub-blocks, its token lists)."""
    w = BitWriter()
    if zlib_header:
        w.put(0x78, 8)
        w.put(0x01, 8)
    nsub = -(-len(seg) // SUB)
    if kind == 'stored':
        for b in range(0, len(seg), 65535):
            piece = seg[b:b + 65535]
            w.put(1 if last and b + 65535 >= len(seg) else 0, 8)
            w.put(len(piece), 16)
            w.put(len(piece) ^ 0xffff, 16)
            for v in piece:
                w.put(v, 8)
        return w.tobytes(), [0] * nsub, None
    toks = tokenize(seg, distances)
    if kind == 'fixed':
        lit, dist = FIXED_LIT, FIXED_DIST
        w.put(0, 1)
        w.put(1, 2)
    else:
        lf, df = [0] * 286, [0] * 30
        lf[256] = 1
        for t in (t for sub in toks for t in sub):
            if t[0] == 'L':
                lf[t[1]] += 1
            else:
                lf[_len_symbol(t[1])[0]] += 1
                df[_dist_symbol(t[2])[0]] += 1
        for d in range(30):                                       # fewer than two distance codes in use: dummies, so that the code is complete
            if sum(1 for f in df if f) < 2 and df[d] == 0:
                df[d] = 1
        lit, dist = code_lengths(lf), code_lengths(df)
        hlit, hdist = max(s for s in range(286) if lit[s]) + 1, max(s for s in range(30) if dist[s]) + 1
        hlit = max(hlit, 257)
        lit, dist = lit[:hlit], dist[:hdist]
        w.put(0, 1)
        w.put(2, 2)
        w.put(hlit - 257, 5)
        w.put(hdist - 1, 5)
        w.put(15, 4)
        for k in range(19):                                       # code-length code: 16, 17, 18 unused, every length 0 .. 15 a flat 4-bit code
            w.put(0 if k < 3 else 4, 3)
        for n in lit + dist:
            w.code((4, n))
    lc, dc = _codes(lit), _codes(dist)
    entries = []
    for sub in toks:
        entries.append(len(w.bits))
        for t in sub:
            if t[0] == 'L':
                w.code(lc[t[1]])
            else:
                s, eb, ev = _len_symbol(t[1])
                w.code(lc[s])
                w.put(ev, eb)
                s, eb, ev = _dist_symbol(t[2])
                w.code(dc[s])
                w.put(ev, eb)
    w.code(lc[256])
    w.put(1 if last else 0, 1)                                    # the empty stored block that ends the chunk byte-aligned
    w.put(0, 2)
    w.align()
    w.put(0, 16)
    w.put(0xffff, 16)
    return w.tobytes(), entries, toks


def default_distances(W):
    row = 1 + 3 * W
    return [d for d in dict.fromkeys((1, 2, 3, 4, 6, 9, 12, row - 3, row, row + 3, 2 * row, 5 * row + 1)) if 1 <= d <= 32768]


class Packed(object):
    """What write_packed_png returns: `data` the file; `stream` the filtered scanline stream; `types` the filter type per row; `table` [(offset of the
    IDAT data, bytes, kind, first index entry)]; `index_off` the offset of the ldIX data; `entries` the index entries per segment; `tokens` per segment
    (None for a stored one); `row_starts` by ldetr_png_scan's rule."""


def index_payload(types, entries, version=1, seg=SEG, sub=SUB):
    return struct.pack('>III', version, seg, sub) + bytes(int(t) for t in types) + b''.join(struct.pack('>I', e) for es in entries for e in es)


def write_packed_png(pixels, kinds='dynamic', distances=None, check=True, schedule=None):
    """uint8 [H, W, 3] + a block type per segment ('stored' | 'fixed' | 'dynamic', one name for all or a sequence cycled through) -> Packed.  Row filters
    by the encoder's rule, or row y by schedule[y % len(schedule)]."""
    H, W, _ = pixels.shape
    if schedule is None:
        types, stream = E.filter_choice(pixels)
    else:
        types, stream = np.array([schedule[y % len(schedule)] for y in range(H)]), P.filter_rows(pixels, schedule)
    segs = segments(len(stream))
    kinds = [kinds] * len(segs) if isinstance(kinds, str) else [kinds[i % len(kinds)] for i in range(len(segs))]
    distances = default_distances(W) if distances is None else distances
    out = Packed()
    out.stream, out.types, out.entries, out.tokens, payloads = stream, types, [], [], []
    for i, (a, b) in enumerate(segs):
        z, entries, toks = deflate_segment(stream[a:b], kinds[i], i == len(segs) - 1, i == 0, distances)
        payloads.append(z + (struct.pack('>I', zlib.adler32(stream)) if i == len(segs) - 1 else b''))
        out.entries.append(entries)
        out.tokens.append(toks)
    out.data, out.table, out.index_off = assemble(W, H, index_payload(types, out.entries), payloads, kinds)
    out.row_starts, last = [], 0
    for y, t in enumerate(types):
        if y == 0 or (t <= 1 and y - last >= 64):
            out.row_starts.append(y)
            last = y
    if check:
        assert zlib.decompress(E.idat(out.data)) == stream
        assert np.array_equal(E.pillow_decode(out.data), pixels)
    return out


def assemble(W, H, index, payloads, kinds):
    """-> (file bytes, segment table, offset of the ldIX data)."""
    head = E.SIGNATURE + P.chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0))
    parts, table = [head, P.chunk(b'ldIX', index)], []
    pos, first = len(head) + 12 + len(index), 0
    for z, kind in zip(payloads, kinds):
        table.append((pos + 8, len(z), KINDS[kind], first))
        parts.append(P.chunk(b'IDAT', z))
        pos += 12 + len(z)
        first += SEG // SUB
    parts.append(P.chunk(b'IEND', b''))
    return b''.join(parts), table, len(head) + 8


def replace_index(packed, index):
    """The file with another ldIX payload (CRC refreshed): for the scan's error cases."""
    at = packed.index_off - 8
    n, = struct.unpack('>I', packed.data[at:at + 4])
    return packed.data[:at] + P.chunk(b'ldIX', index) + packed.data[at + 12 + n:]


def set_entry(data, packed, segment, k, value):
    """The file bytes with index entry k of a segment overwritten in place (the chunk's CRC is left stale: the device path does not read it)."""
    at = packed.index_off + 12 + len(packed.types) + 4 * (packed.table[segment][3] + k)
    return data[:at] + struct.pack('>I', value) + data[at + 4:]


def hostcheck_job(data, table, index_off, H, W, stream):
    """The job file of tools/png_inflate_hostcheck.cpp."""
    return (b'LDIXJOB1' + struct.pack('<5q', H, W, len(table), len(data), index_off) + b''.join(struct.pack('<4q', *row) for row in table) + bytes(data) + bytes(stream))
