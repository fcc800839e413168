"""Layout grids rendered on the device: the reference's `save_image` (util.py:115-141) and its `convert_layout_to_image` (util.py:85-112).

The reference builds every grid cell in Python: `boxes[i][mask]` on device tensors, one `ImageDraw.rectangle` per element on a page-sized
canvas, a PIL resize, `ToTensor`, `make_grid`, `save_image`.  `layout_grid` does all of it in ONE launch (csrc/layout_raster.hip) and returns
the uint8 grid the reference's PNG holds, bit for bit (the rule is DESIGN.md §13); `save_png` is one device-to-host copy and the PNG encoder.
There is no CPU fallback: without the HIP library or a GPU tensor it raises.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .hip import core

FILTER_BILINEAR, FILTER_LANCZOS = 0, 1
MAX_BOXES = 16

_table_cache = {}   # (in, out) -> int32 [2 * out + ksize * out] host table
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


def bilinear_coeffs(in_size, out_size, filter=FILTER_BILINEAR):
    """(bounds [out, 2], weights [ksize, out], ksize) of Pillow's window for in_size -> out_size, host int32 (ldetr_resample_coeffs_filter)."""
    lib = _lib.load()
    ks = ctypes.c_int(0)
    core.check(lib.ldetr_resample_coeffs_filter(filter, in_size, out_size, None, None, 0, ctypes.byref(ks)), 'resample_coeffs_filter')
    bounds = np.zeros((out_size, 2), np.int32)
    weights = np.zeros((ks.value, out_size), np.int32)
    core.check(lib.ldetr_resample_coeffs_filter(filter, in_size, out_size, bounds.ctypes.data_as(ctypes.c_void_p), weights.ctypes.data_as(ctypes.c_void_p),
                                                weights.size, ctypes.byref(ks)), 'resample_coeffs_filter')
    return bounds, weights, ks.value


def _coeff_pool(pairs, device):
    """One device pool holding the table of every distinct (in, out) pair of a grid; cached per set of pairs."""
    key = (tuple(pairs), str(device))
    hit = _pool_cache.get(key)
    if hit is not None:
        return hit
    parts, where, at = [], {}, 0
    for pair in pairs:
        t = _table_cache.get(pair)
        if t is None:
            b, w, ks = bilinear_coeffs(*pair)
            t = _table_cache[pair] = (np.concatenate([b.reshape(-1), w.reshape(-1)]), ks)
        where[pair] = (at, t[1])
        parts.append(t[0])
        at += t[0].size
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
    B, N = int(bbox.shape[0]), int(bbox.shape[1])
    S = int(canvas)
    if N < 1 or N > MAX_BOXES:
        raise ValueError(f'layout_grid: 1 <= N <= {MAX_BOXES} boxes per layout (got {N})')
    if S < 2 or S % 2 != 0:
        raise ValueError(f'layout_grid: the canvas size must be even (got {canvas}); the reference fails in torch.stack otherwise')
    if nrow is not None and int(nrow) < 1:
        raise ValueError('layout_grid: nrow must be positive')
    dev = bbox.device
    if B == 0:
        return torch.zeros((0, 0, 3), dtype=torch.uint8, device=dev)
    valid_h = _host(valid, np.uint8).reshape(B, N)
    labels_h = _host(labels, np.int32).reshape(B, N)
    pal = _host(colors, np.uint8).reshape(-1, 3)
    wh = _host(page_wh, np.int32)
    wh = np.ascontiguousarray(np.broadcast_to(wh.reshape(1, 2), (B, 2))) if wh.size == 2 else wh.reshape(B, 2)
    if labels_h[valid_h != 0].size and (labels_h[valid_h != 0].min() < 0 or labels_h[valid_h != 0].max() >= pal.shape[0]):
        raise ValueError(f'layout_grid: label outside the palette of {pal.shape[0]} colours')
    pairs, cell_pairs = [], []
    for W, H in wh.tolist():
        if W < 1 or H < 1:
            raise ValueError(f'layout_grid: bad page size {W} x {H}')
        Wn, Hn = cell_size(W, H, S)
        if Wn < 1 or Hn < 1:
            raise ValueError(f'layout_grid: a {W} x {H} page leaves no pixel at canvas size {S}')
        hp, vp = ((W, Wn) if W != Wn else None), ((H, Hn) if H != Hn else None)
        cell_pairs.append((hp, vp))
        for pr in (hp, vp):
            if pr is not None and pr not in pairs:
                pairs.append(pr)
    pool, where = _coeff_pool(sorted(pairs), dev)
    cc = np.asarray([[where[hp][0] if hp else -1, where[hp][1] if hp else 0, where[vp][0] if vp else -1, where[vp][1] if vp else 0]
                     for hp, vp in cell_pairs], np.int64)
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
    Hg, Wg, _, _ = grid_shape(B, S, nrow)
    bb = core.f32c(bbox)
    cells = torch.empty(B * 32, dtype=torch.int32, device=dev)
    out = torch.empty((Hg, Wg, 3), dtype=torch.uint8, device=dev)
    a.bbox, a.valid, a.labels, a.palette, a.page_wh = bb.data_ptr(), valid_h.ctypes.data, labels_h.ctypes.data, pal.ctypes.data, wh.ctypes.data
    a.coeffs, a.coeffs_len, a.cell_coeffs = pool.data_ptr(), pool.numel(), cc.ctypes.data
    a.cells_dev, a.out = cells.data_ptr(), out.data_ptr()
    core.check(core.lib().ldetr_layout_raster_u8(ctypes.byref(a), core.stream()), 'layout_raster')
    del keep
    return out


def save_png(grid, path):
    """Write a uint8 [H, W, 3] grid as a PNG: one device-to-host copy, then PIL encodes."""
    import PIL.Image
    if grid.dtype != torch.uint8 or grid.ndim != 3 or grid.shape[2] != 3:
        raise ValueError('save_png: expected a uint8 [H, W, 3] grid')
    PIL.Image.fromarray(grid.detach().cpu().numpy(), 'RGB').save(path)
