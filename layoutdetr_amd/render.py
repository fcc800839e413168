"""Layout grids rendered on the device: the reference's `save_image` (util.py:115-141) and its `convert_layout_to_image` (util.py:85-112).

The reference builds every grid cell in Python: `boxes[i][mask]` on device tensors, one `ImageDraw.rectangle` per element on a page-sized
canvas, a PIL resize, `ToTensor`, `make_grid`, `save_image`.  `layout_grid` does all of it in ONE launch (csrc/layout_raster.hip) and returns
the uint8 grid the reference's PNG holds, bit for bit (the rule is DESIGN.md §13); `save_png` is one device-to-host copy and the PNG encoder, or, on
request, `encode_png`: the PNG file built on the device (csrc/png_encode.hip) and only its bytes copied.
There is no CPU fallback: without the HIP library or a GPU tensor it raises.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .hip import core
from .pil_coeffs import FILTER_BILINEAR, coeff_table

MAX_BOXES = 16

_pool_cache = {}    # (tuple of (in, out), device) -> (device pool, {pair: (offset, ksize)})


def cell_size(W, H, canvas):
    """(Wn, Hn): what a W x H page is resized to inside a canvas x canvas cell (util.py:105-110), in double arithmetic as Python evaluates it."""
    if W > H:
        return canvas, int(float(H) / float(W) * float(canvas)) // 2 * 2
    return int(float(W) / float(H) * float(canvas)) // 2 * 2, canvas


def grid_shape(B, canvas, nrow=None):
    """(Hg, Wg, xmaps, ymaps) of torchvision's make_grid(padding=2) for B cells; B == 1 is the cell itself."""
    if B == 1:
        return canvas, canvas, 1, 1
    if nrow is None:
        nrow = int(math.ceil(math.sqrt(B)))
    xmaps = min(int(nrow), B)
    ymaps = int(math.ceil(float(B) / xmaps))
    return ymaps * (canvas + 2) + 2, xmaps * (canvas + 2) + 2, xmaps, ymaps


def _coeff_pool(pairs, device):
    """One device pool holding the table of every distinct (in, out) pair of a grid; cached per set of pairs."""
    key = (tuple(pairs), str(device))
    hit = _pool_cache.get(key)
    if hit is not None:
        return hit
    parts, where, at = [], {}, 0
    for pair in pairs:
        b, w, ks = coeff_table(pair[0], pair[1], FILTER_BILINEAR)
        where[pair] = (at, ks)
        parts += [b.reshape(-1), w.reshape(-1)]
        at += b.size + w.size
    pool = torch.from_numpy(np.concatenate(parts) if parts else np.zeros(1, np.int32)).to(device)
    if len(_pool_cache) > 64:
        _pool_cache.clear()
    _pool_cache[key] = (pool, where)
    return pool, where


class PageSet(object):
    """Decoded uint8 pages of different sizes in ONE device buffer + the table (byte offset, W, H) the kernel reads them through."""

    def __init__(self, pages):
        pages = [pages] if torch.is_tensor(pages) and pages.ndim == 3 else list(pages)
        core.require_gpu(*pages)
        table, at = [], 0
        for p in pages:
            if p.dtype != torch.uint8 or p.ndim != 3 or p.shape[2] != 3:
                raise ValueError('PageSet: every page must be uint8 [H, W, 3]')
            table.append((at, int(p.shape[1]), int(p.shape[0])))
            at += p.numel()
        self.table = np.asarray(table, np.int64).reshape(-1, 3)
        self.buffer = torch.cat([p.contiguous().reshape(-1) for p in pages]) if len(pages) != 1 else pages[0].contiguous().reshape(-1)

    def __len__(self):
        return self.table.shape[0]


def _host(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x).astype(dtype))


def _grid_args(who, what, bbox, canvas, nrow, why_even=''):
    """(B, N, S) of a grid call after the checks layout_grid and image_grid share."""
    B, N = int(bbox.shape[0]), int(bbox.shape[1])
    S = int(canvas)
    if N < 1 or N > MAX_BOXES:
        raise ValueError(f'{who}: 1 <= N <= {MAX_BOXES} {what} per layout (got {N})')
    if S < 2 or S % 2 != 0:
        raise ValueError(f'{who}: the canvas size must be even (got {canvas}){why_even}')
    if nrow is not None and int(nrow) < 1:
        raise ValueError(f'{who}: nrow must be positive')
    return B, N, S


def _page_wh(page_wh, B):
    """page_wh, (W, H) for every cell or [B, 2], as a host int32 [B, 2] array."""
    wh = _host(page_wh, np.int32)
    return np.ascontiguousarray(np.broadcast_to(wh.reshape(1, 2), (B, 2))) if wh.size == 2 else wh.reshape(B, 2)


def _grid_buffers(who, wh, S, nrow, dev, cell_ints):
    """What a raster entry needs beside its kind's own arrays: the device pool of the cells' coefficient tables, its rows per cell (`cc`: offset
    and ksize of the W -> Wn and of the H -> Hn table, offset -1 for a pass whose sizes agree), the descriptor scratch and the grid [Hg, Wg, 3].
    (image_grid has rejected a page size below 1 before it gets here: it needs the sizes earlier, for the paste rectangles.)"""
    pairs, cell_pairs = [], []
    for W, H in wh.tolist():
        if W < 1 or H < 1:
            raise ValueError(f'{who}: bad page size {W} x {H}')
        Wn, Hn = cell_size(W, H, S)
        if Wn < 1 or Hn < 1:
            raise ValueError(f'{who}: a {W} x {H} page leaves no pixel at canvas size {S}')
        hp, vp = ((W, Wn) if W != Wn else None), ((H, Hn) if H != Hn else None)
        cell_pairs.append((hp, vp))
        for pr in (hp, vp):
            if pr is not None and pr not in pairs:
                pairs.append(pr)
    pool, where = _coeff_pool(sorted(pairs), dev)
    cc = np.asarray([[where[hp][0] if hp else -1, where[hp][1] if hp else 0, where[vp][0] if vp else -1, where[vp][1] if vp else 0]
                     for hp, vp in cell_pairs], np.int64)
    Hg, Wg, _, _ = grid_shape(len(cell_pairs), S, nrow)
    cells = torch.empty(len(cell_pairs) * cell_ints, dtype=torch.int32, device=dev)
    return pool, cc, cells, torch.empty((Hg, Wg, 3), dtype=torch.uint8, device=dev)


def layout_grid(bbox, valid, labels, colors, page_wh, pages=None, page_index=None, canvas=128, nrow=None):
    """uint8 [Hg, Wg, 3] device tensor: the pixels of the PNG the reference's save_image(bbox, labels, valid, colors, path, W_page, H_page,
    size_canvas=canvas, nrow=nrow) writes, in one launch.

    bbox [B, N, 4] fp32 (xc, yc, w, h) in GPU memory, N <= 16; valid, labels [B, N] (read on the host: pass CPU tensors to avoid a device-to-host
    copy); colors: one RGB triple per label; page_wh: (W, H) for every cell or [B, 2].  pages (optional): a PageSet, or uint8 [H, W, 3] device
    tensors, drawn on instead of a white page; page_index [B] names each cell's page (-1 = white; several cells may share one), default
    cell b -> page b."""
    core.require_gpu(bbox)
    if bbox.ndim != 3 or bbox.shape[-1] != 4:
        raise ValueError('layout_grid: bbox must be [B, N, 4]')
    B, N, S = _grid_args('layout_grid', 'boxes', bbox, canvas, nrow, '; the reference fails in torch.stack otherwise')
    dev = bbox.device
    if B == 0:
        return torch.zeros((0, 0, 3), dtype=torch.uint8, device=dev)
    valid_h = _host(valid, np.uint8).reshape(B, N)
    labels_h = _host(labels, np.int32).reshape(B, N)
    pal = _host(colors, np.uint8).reshape(-1, 3)
    wh = _page_wh(page_wh, B)
    if labels_h[valid_h != 0].size and (labels_h[valid_h != 0].min() < 0 or labels_h[valid_h != 0].max() >= pal.shape[0]):
        raise ValueError(f'layout_grid: label outside the palette of {pal.shape[0]} colours')
    pool, cc, cells, out = _grid_buffers('layout_grid', wh, S, nrow, dev, 32)
    a = _lib.LayoutRasterArgs()
    a.struct_bytes = ctypes.sizeof(_lib.LayoutRasterArgs)
    a.B, a.N, a.S, a.nrow, a.n_colors = B, N, S, 0 if nrow is None else int(nrow), pal.shape[0]
    keep = [valid_h, labels_h, pal, wh, cc]
    if pages is not None:
        if not isinstance(pages, PageSet):
            pages = PageSet(pages)
        core.require_gpu(pages.buffer)
        pi = np.arange(B, dtype=np.int32) if page_index is None else _host(page_index, np.int32).reshape(-1)
        if pi.size != B:
            raise ValueError('layout_grid: page_index must name one page per cell')
        if page_index is None and len(pages) != B:
            raise ValueError('layout_grid: page_index is needed when the number of pages differs from the number of cells')
        keep += [pi, pages.table]
        a.n_pages, a.pages, a.pages_bytes = len(pages), pages.buffer.data_ptr(), pages.buffer.numel()
        a.page_table, a.page_index = pages.table.ctypes.data, pi.ctypes.data
    bb = core.f32c(bbox)
    a.bbox, a.valid, a.labels, a.palette, a.page_wh = bb.data_ptr(), valid_h.ctypes.data, labels_h.ctypes.data, pal.ctypes.data, wh.ctypes.data
    a.coeffs, a.coeffs_len, a.cell_coeffs = pool.data_ptr(), pool.numel(), cc.ctypes.data
    a.cells_dev, a.out = cells.data_ptr(), out.data_ptr()
    core.check(core.lib().ldetr_layout_raster_u8(ctypes.byref(a), core.stream()), 'layout_raster')
    del keep
    return out


PNG_ENCODE_SEGMENT = 65536   # csrc/png_encode.hip PE_SEG: bytes of filtered scanline stream per deflate segment (one workgroup, one IDAT chunk)
PNG_ENCODE_SLOT = 2 * PNG_ENCODE_SEGMENT + 512   # PE_SLOT: the most a segment's deflate bytes take under a forced block type
PNG_ENV = 'LDETR_SNAPSHOT_PNG'                   # which encoder save_png uses when it is not told: 'pillow' (default) or 'device'
_BLOCKS = {'auto': 0, 'stored': 1, 'fixed': 2, 'dynamic': 3}
BLOCK_NAMES = ('stored', 'fixed', 'dynamic')     # block type column of the segment table


def _check_grid_size(H, W):
    if not (1 <= int(W) <= MAX_RESIZE and 1 <= int(H) <= MAX_RESIZE):
        raise ValueError(f'png encode: a {W} x {H} grid is outside [1, {MAX_RESIZE}] x [1, {MAX_RESIZE}]')


def png_encode_bound(H, W):
    """(file bytes, workspace bytes): the largest file encode_png(blocks='auto' | 'stored') returns for an H x W grid (every segment stored) and the
    device workspace one call takes (ldetr_png_encode_bound; host arithmetic only)."""
    _check_grid_size(H, W)
    out, ws = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().ldetr_png_encode_bound(int(H), int(W), ctypes.byref(out), ctypes.byref(ws)), 'png_encode_bound')
    return out.value, ws.value


def png_encode_segments(H, W):
    """[(first byte, end byte)]: how the filtered scanline stream of H (1 + 3 W) bytes is cut into deflate segments; no back-reference crosses a
    seam, and each segment is one IDAT chunk."""
    _check_grid_size(H, W)
    total = int(H) * (1 + 3 * int(W))
    return [(a, min(a + PNG_ENCODE_SEGMENT, total)) for a in range(0, total, PNG_ENCODE_SEGMENT)]


def png_index_bytes(H, W):
    """What encode_png(index=True) adds to both of png_encode_bound's figures: the ldIX chunk, rounded up to 16 bytes (ldetr_png_index_bytes; host
    arithmetic only)."""
    _check_grid_size(H, W)
    out = ctypes.c_int64(0)
    _lib.check(_lib.load().ldetr_png_index_bytes(int(H), int(W), ctypes.byref(out)), 'png_index_bytes')
    return out.value


def encode_png(grid, blocks='auto', filter='auto', return_stats=False, index=False):
    """A uint8 [H, W, 3] grid in GPU memory -> the bytes of its PNG file as a host uint8 tensor, encoded on the device (csrc/png_encode.hip, DESIGN.md
    §17): three launches, then one 8-byte copy (the length) and one copy of exactly that many bytes.  blocks: 'auto' takes the smallest of a stored,
    a fixed-Huffman and a dynamic-Huffman block per 64 KiB segment; 'stored' / 'fixed' / 'dynamic' force one type ('stored' gives a file
    dataset_layoutganpp.scan_png finds eligible).  filter: 'auto' picks per row by the minimum sum of absolute residuals, 0..4 force a type.
    return_stats=True: (bytes, stats) with stats['segments'] an int64 [n, 4] array of (first byte, end byte, block type 0 / 1 / 2, chunk bytes).
    index=True adds the ancillary ldIX chunk in front of the first IDAT (the filter type of every row and the bit offset of every
    512-byte sub-block's first token), which lets dataset_layoutganpp.scan_png(packed=True) / decode_pages inflate the file on the device; every other
    byte of the file is the same, and decoders that do not know the chunk skip it.
    There is no CPU path: a CPU tensor raises."""
    core.require_gpu(grid)
    if grid.dtype != torch.uint8 or grid.ndim != 3 or grid.shape[2] != 3:
        raise ValueError('encode_png: expected a uint8 [H, W, 3] grid')
    if blocks not in _BLOCKS:
        raise ValueError(f"encode_png: blocks must be one of {sorted(_BLOCKS)} (got {blocks!r})")
    if filter != 'auto' and filter not in (0, 1, 2, 3, 4):
        raise ValueError(f"encode_png: filter must be 'auto' or 0..4 (got {filter!r})")
    H, W = int(grid.shape[0]), int(grid.shape[1])
    _check_grid_size(H, W)
    bound, ws_bytes = png_encode_bound(H, W)
    nseg = len(png_encode_segments(H, W))
    cap = bound if _BLOCKS[blocks] < 2 else 64 + nseg * (12 + PNG_ENCODE_SLOT)
    if index:
        extra = png_index_bytes(H, W)
        bound, ws_bytes, cap = bound + extra, ws_bytes + extra, cap + extra
    dev = grid.device
    src = grid.contiguous()
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    small = torch.zeros(1 + 4 * nseg, dtype=torch.int64, device=dev)          # [total length | segment table]
    a = _lib.PngEncodeArgs(struct_bytes=ctypes.sizeof(_lib.PngEncodeArgs), H=H, W=W, blocks=_BLOCKS[blocks], filter=-1 if filter == 'auto' else int(filter), reserved=1 if index else 0,
                           src=src.data_ptr(), out=out.data_ptr(), out_capacity=cap, total_bytes=small.data_ptr(),
                           workspace=ws.data_ptr(), workspace_bytes=ws_bytes, seg_table=small.data_ptr() + 8, seg_table_rows=nseg)
    core.check(core.lib().ldetr_png_encode_u8(ctypes.byref(a), core.stream()), 'png_encode_u8')
    if return_stats:
        small_h = small.cpu()
        n = int(small_h[0])
    else:
        n = int(small[0].item())
    if n <= 0 or n > cap:
        raise RuntimeError(f'encode_png: the file needs {-n} bytes, the buffer holds {cap}')
    data = out[:n].cpu()
    if return_stats:
        return data, dict(segments=small_h[1:].reshape(nseg, 4).numpy().copy(), bytes_to_host=n + small_h.numel() * 8, bound=bound)
    return data


def save_png(grid, path, encoder=None, index=False):
    """Write a uint8 [H, W, 3] grid as a PNG.  encoder 'pillow' (the default): one device-to-host copy of the pixels, then PIL encodes; 'device':
    encode_png on the GPU, only the file's bytes cross to the host.  None reads the environment variable LDETR_SNAPSHOT_PNG (unset: 'pillow').
    index=True (the device encoder only): the file carries the ldIX chunk of encode_png(index=True)."""
    if grid.dtype != torch.uint8 or grid.ndim != 3 or grid.shape[2] != 3:
        raise ValueError('save_png: expected a uint8 [H, W, 3] grid')
    if encoder is None:
        import os
        encoder = os.environ.get(PNG_ENV, '') or 'pillow'
        if encoder not in ('pillow', 'device'):
            raise ValueError(f"{PNG_ENV} must be 'pillow' or 'device' (got {encoder!r})")
    elif encoder not in ('pillow', 'device'):
        raise ValueError(f"save_png: encoder must be 'pillow', 'device' or None for {PNG_ENV} (got {encoder!r})")
    if index and encoder != 'device':
        raise ValueError("save_png: index=True needs encoder='device' (Pillow writes no ldIX chunk)")
    if encoder == 'device':
        data = encode_png(grid, index=index).numpy()
        with open(path, 'wb') as f:
            f.write(memoryview(data))
        return
    import PIL.Image
    PIL.Image.fromarray(grid.detach().cpu().numpy(), 'RGB').save(path)


# ---- the `images` kinds: text patches pasted at the generated boxes (util.py:144-325; DESIGN.md §13 rules 8-12) ----

IMAGE_CANVAS = 1024          # save_real_image's default size_canvas
MAX_RESIZE = 16384           # csrc/patch_resize.hip: largest source / target axis

_axis_cache = {}    # (in, out) -> int32 words of one axis table


def resize_axis_table(n_in, n_out):
    """One axis of skimage.transform.resize(anti_aliasing=True) as the kernel reads it (rule 10), int32 words: [r][2r + 1 Gaussian weights][i0][i1][w0][w1],
    built in double, the weights stored as fp32 bits."""
    key = (int(n_in), int(n_out))
    hit = _axis_cache.get(key)
    if hit is not None:
        return hit
    n_in, n_out = key
    f = n_in / n_out
    sigma = max(0.0, (f - 1.0) / 2.0)
    r = int(4.0 * sigma + 0.5) if sigma > 0 else 0
    if r > 0:
        k = np.arange(-r, r + 1, dtype=np.float64)
        g = np.exp(-0.5 * (k / sigma) ** 2)
        g = g / g.sum()
    else:
        g = np.ones(1, np.float64)
    c = (np.arange(n_out, dtype=np.float64) + 0.5) * f - 0.5
    i0 = np.floor(c)
    t = c - i0

    def mirror(i):
        if n_in == 1:
            return np.zeros_like(i, dtype=np.int64)
        p = 2 * (n_in - 1)
        m = np.mod(i.astype(np.int64), p)
        return np.where(m >= n_in, p - m, m)
    words = np.concatenate([np.asarray([r], np.int32), g.astype(np.float32).view(np.int32), mirror(i0).astype(np.int32), mirror(i0 + 1).astype(np.int32),
                            (1.0 - t).astype(np.float32).view(np.int32), t.astype(np.float32).view(np.int32)])
    if len(_axis_cache) > 4096:
        _axis_cache.clear()
    _axis_cache[key] = words
    return words


class PatchSet(object):
    """The uint8 crops of a grid's elements (LayoutDataset.patch_crops: rule 8) in ONE device buffer + the table [cells, N, 3] = (byte offset, w, h)
    the resize jobs are read through; offset -1: the element has no drawable crop.  `crops`: per cell a list of N entries, uint8 [h, w, 3] arrays
    (numpy or torch, host or device) or None."""

    def __init__(self, crops, device):
        crops = [list(c) for c in crops]
        n = max([len(c) for c in crops] + [1])
        table = np.full((len(crops), n, 3), -1, np.int64)
        parts, at = [], 0
        for b, cell in enumerate(crops):
            for i, c in enumerate(cell):
                if c is None:
                    continue
                c = torch.as_tensor(c)
                if c.dtype != torch.uint8 or c.ndim != 3 or c.shape[2] != 3 or c.shape[0] < 1 or c.shape[1] < 1:
                    raise ValueError('PatchSet: every crop must be a non-empty uint8 [h, w, 3]')
                table[b, i] = (at, int(c.shape[1]), int(c.shape[0]))
                parts.append(c.contiguous().reshape(-1))
                at += c.numel()
        self.table = table
        if parts and all(p.device.type == 'cpu' for p in parts):
            self.buffer = torch.cat(parts).to(device)                 # one upload
        else:
            self.buffer = torch.cat([p.to(device) for p in parts]) if parts else torch.zeros(1, dtype=torch.uint8, device=device)
        core.require_gpu(self.buffer)

    def __len__(self):
        return self.table.shape[0]


def paste_rects(bbox_fake, page_wh):
    """Rule 9 on host arrays: int64 [B, N, 4] = (x1, y1, x2, y2), the fp32 corners (xc -+ w / 2) * W, (yc -+ h / 2) * H rounded half to even
    (util.py:167-169); a NaN corner gives an empty rectangle."""
    b = np.asarray(bbox_fake, np.float32)
    wh = np.asarray(page_wh, np.float32).reshape(-1, 1, 2)
    two = np.float32(2)
    with np.errstate(all='ignore'):
        xc, yc, w, h = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
        c = np.stack([(xc - w / two) * wh[..., 0], (yc - h / two) * wh[..., 1], (xc + w / two) * wh[..., 0], (yc + h / two) * wh[..., 1]], -1)
        assert c.dtype == np.float32
        bad = np.isnan(c).any(-1)
        r = np.clip(np.rint(np.nan_to_num(c, nan=0.0)).astype(np.float64), -2 ** 30, 2 ** 30).astype(np.int64)
    r[bad] = 0
    return r


class _ResizeJobs(object):
    """The job list of ONE ldetr_patch_resize_u8 launch: rows (source buffer, src offset, h, w, dst offset, h', w', axis tables) + the pool of the
    axis tables they name."""

    def __init__(self):
        self.jobs, self.axis_at, self.pool, self.pool_len, self.dst_bytes = [], {}, [], 0, 0

    def _table(self, n_in, n_out):
        key = (n_in, n_out)
        if key not in self.axis_at:
            words = resize_axis_table(n_in, n_out)
            self.axis_at[key] = self.pool_len
            self.pool.append(words)
            self.pool_len += words.size
        return self.axis_at[key]

    def add(self, buf, off, h, w, ho, wo):
        """-> the byte offset of the [ho, wo, 3] result in the output buffer."""
        if min(h, w, ho, wo) < 1 or max(h, w, ho, wo) > MAX_RESIZE:
            raise ValueError(f'patch resize: {w} x {h} -> {wo} x {ho}: every axis must be in [1, {MAX_RESIZE}]')
        at = self.dst_bytes
        self.jobs.append((buf, off, h, w, at, ho, wo, self._table(h, ho), self._table(w, wo)))
        self.dst_bytes += ho * wo * 3
        return at

    def launch(self, src0, src1, dev):
        """uint8 device buffer of dst_bytes bytes (at least 1), written by one launch."""
        pixels = torch.empty(max(self.dst_bytes, 1), dtype=torch.uint8, device=dev)
        if not self.jobs:
            return pixels
        jobs_h = np.ascontiguousarray(np.asarray(self.jobs, np.int64).reshape(-1, 9))
        tables_h = np.ascontiguousarray(np.concatenate(self.pool))
        tables_d = torch.from_numpy(tables_h).to(dev)
        jobs_d = torch.empty(len(self.jobs) * 16, dtype=torch.int32, device=dev)
        a = _lib.PatchResizeArgs()
        a.struct_bytes, a.n_jobs = ctypes.sizeof(_lib.PatchResizeArgs), len(self.jobs)
        a.src0, a.src0_bytes = src0.data_ptr(), src0.numel()
        if src1 is not None:
            a.src1, a.src1_bytes = src1.data_ptr(), src1.numel()
        a.dst, a.dst_bytes = pixels.data_ptr(), pixels.numel()
        a.jobs, a.tables, a.tables_host, a.tables_len, a.jobs_dev = jobs_h.ctypes.data, tables_d.data_ptr(), tables_h.ctypes.data, tables_h.size, jobs_d.data_ptr()
        core.check(core.lib().ldetr_patch_resize_u8(ctypes.byref(a), core.stream()), 'patch_resize')
        return pixels


def resize_u8(images, sizes):
    """skimage.transform.resize(im, (h', w'), anti_aliasing=True) of every uint8 [h, w, 3] device tensor of `images` to its (h', w') of `sizes`, by rule 10
    of DESIGN.md §13, in ONE launch -> list of uint8 [h', w', 3] device tensors (views of one buffer)."""
    images = list(images)
    core.require_gpu(*images)
    if not images:
        return []
    pages = PageSet(images)
    rj = _ResizeJobs()
    at = [rj.add(0, int(off), int(h), int(w), int(ho), int(wo)) for (off, w, h), (ho, wo) in zip(pages.table.tolist(), sizes)]
    pixels = rj.launch(pages.buffer, None, images[0].device)
    return [pixels[o:o + int(ho) * int(wo) * 3].view(int(ho), int(wo), 3) for o, (ho, wo) in zip(at, sizes)]


def image_grid(bbox_fake, bbox_real, valid, patches, page_wh, backgrounds=None, canvas=IMAGE_CANVAS, nrow=None, patch_index=None, background_index=None):
    """uint8 [Hg, Wg, 3] device tensor: the pixels the reference's save_real_image (backgrounds=None, util.py:207-231) or
    save_real_image_with_background (util.py:298-325) grid holds, by the rule of DESIGN.md §13 (rules 8-12), in two launches: one batched
    anti-aliased resize of every element crop (and page background) to its paste size, one compositing raster.

    bbox_fake [B, N, 4] fp32 in GPU memory (ONE device-to-host copy of it gives the paste rectangles); bbox_real [B, N, 4]: the boxes the crops were
    made from, read on the host only to check the crop sizes (pass a CPU tensor to avoid a second small copy); valid [B, N] (host);
    patches: a PatchSet of the crops LayoutDataset.patch_crops made from bbox_real; page_wh: (W, H) or [B, 2]; backgrounds: a PageSet (or uint8
    [h, w, 3] device tensors) of any size, resized to the page.  patch_index / background_index [B]: the PatchSet cell / page each grid cell
    uses (default b -> b; several cells may share one).  There is no CPU fallback."""
    core.require_gpu(bbox_fake)
    if bbox_fake.ndim != 3 or bbox_fake.shape[-1] != 4 or bbox_real.shape != bbox_fake.shape:
        raise ValueError('image_grid: bbox_fake and bbox_real must both be [B, N, 4]')
    if not isinstance(patches, PatchSet):
        raise ValueError('image_grid: patches must be a render.PatchSet')
    B, N, S = _grid_args('image_grid', 'elements', bbox_fake, canvas, nrow)
    dev = bbox_fake.device
    if B == 0:
        return torch.zeros((0, 0, 3), dtype=torch.uint8, device=dev)
    core.require_gpu(patches.buffer)
    valid_h = _host(valid, np.uint8).reshape(B, N).copy()
    wh = _page_wh(page_wh, B)
    if (wh < 1).any():
        raise ValueError('image_grid: bad page size')
    pidx = np.arange(B) if patch_index is None else _host(patch_index, np.int64).reshape(-1)
    if pidx.size != B or (pidx < 0).any() or (pidx >= len(patches)).any() or patches.table.shape[1] < N:
        raise ValueError('image_grid: patch_index must name one PatchSet cell of at least N slots per grid cell')
    rects = paste_rects(core.f32c(bbox_fake).cpu().numpy(), wh)                              # the one device-to-host copy of the generated boxes
    boxes_real = _host(bbox_real, np.float32)
    # rule 8's crop size, to catch a PatchSet that was not made from these real boxes
    with np.errstate(all='ignore'):
        real_wh = np.nan_to_num(boxes_real[..., 2:4] * wh.astype(np.float32).reshape(B, 1, 2), nan=-1.0, posinf=-1.0, neginf=-1.0).astype(np.int64)
    bg_table = None
    if backgrounds is not None:
        if not isinstance(backgrounds, PageSet):
            backgrounds = PageSet(backgrounds)
        core.require_gpu(backgrounds.buffer)
        bidx = np.arange(B) if background_index is None else _host(background_index, np.int64).reshape(-1)
        if bidx.size != B or (bidx < 0).any() or (bidx >= len(backgrounds)).any():
            raise ValueError('image_grid: background_index must name one page per cell')
        bg_table = backgrounds.table[bidx]
    rj, bg_done = _ResizeJobs(), {}
    job = rj.add
    patch_off = np.full((B, N), -1, np.int64)
    page_off = np.full(B, -1, np.int64)
    for b in range(B):
        W, H = int(wh[b, 0]), int(wh[b, 1])
        if bg_table is not None:
            off, bw, bh = (int(v) for v in bg_table[b])
            if (off, W, H) not in bg_done:                            # cells that share a background and a page size share its resize
                bg_done[(off, W, H)] = job(1, off, bh, bw, H, W)
            page_off[b] = bg_done[(off, W, H)]
        for i in range(N):
            off, cw, ch = (int(v) for v in patches.table[pidx[b], i])
            x1, y1, x2, y2 = (int(v) for v in rects[b, i])
            if not valid_h[b, i] or off < 0 or x2 <= x1 or y2 <= y1 or x2 <= 0 or y2 <= 0 or x1 >= W or y1 >= H:
                valid_h[b, i] = 0                                     # draws nothing (rules 8, 9)
                continue
            if (cw, ch) != (int(real_wh[b, i, 0]), int(real_wh[b, i, 1])):
                raise ValueError(f'image_grid: cell {b} slot {i}: the crop is {cw} x {ch}, bbox_real asks for {int(real_wh[b, i, 0])} x {int(real_wh[b, i, 1])}')
            patch_off[b, i] = job(0, off, ch, cw, y2 - y1, x2 - x1)
    cpool, cc, cells, out = _grid_buffers('image_grid', wh, S, nrow, dev, 128)
    lib, st = core.lib(), core.stream()
    pixels = rj.launch(patches.buffer, None if backgrounds is None else backgrounds.buffer, dev)
    rects32 = np.ascontiguousarray(np.clip(rects, -2 ** 30, 2 ** 30).astype(np.int32))
    bb = core.f32c(bbox_fake)
    a = _lib.ImageRasterArgs()
    a.struct_bytes = ctypes.sizeof(_lib.ImageRasterArgs)
    a.B, a.N, a.S, a.nrow = B, N, S, 0 if nrow is None else int(nrow)
    a.bbox, a.valid, a.rects, a.patch_off, a.page_off, a.page_wh = bb.data_ptr(), valid_h.ctypes.data, rects32.ctypes.data, patch_off.ctypes.data, page_off.ctypes.data, wh.ctypes.data
    a.pixels, a.pixels_bytes = pixels.data_ptr(), pixels.numel()
    a.coeffs, a.coeffs_len, a.cell_coeffs = cpool.data_ptr(), cpool.numel(), cc.ctypes.data
    a.cells_dev, a.out = cells.data_ptr(), out.data_ptr()
    core.check(lib.ldetr_image_raster_u8(ctypes.byref(a), st), 'image_raster')
    return out
