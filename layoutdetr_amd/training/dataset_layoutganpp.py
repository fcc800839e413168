"""The reference's dataset (training/dataset_layoutganpp.py) for the gfx950 hot path: zip + `non_image.json` reader.

On-disk format (written by the reference's dataset_tool.py:295-366, read by training/dataset_layoutganpp.py:214-342): one zip
holding `non_image.json` = {"samples": [[base_fname, {bboxes [n][4] (xc, yc, w, h in page units), labels [n], texts [n],
page_label, attr {name, width, height, num_bbox_labels}}], ...]} and per sample `<base>_background_orig.png`,
`<base>_<i>_patch.png`, `<base>_<i>_patch_orig.png`, `<base>_<i>_patch_mask.png` (i < n <= 9).  Every field is padded to
nine slots with a validity mask (`to_dense_batch`, :29-41).

`LayoutDataset(path, background_size=..., mode=...)`, same constructor arguments / properties / item keys as the reference:

* mode='device' (default, the training path): `__getitem__` inflates ONLY the page background PNG (byte-serial entropy
  decoding stays on the host) and ships it as it is, uint8 [H, W, 3] (3 bytes per pixel instead of 12); resize to
  `background_size` + ImageNet normalisation + HWC -> CHW run on the GPU for the whole batch (`background_to_tensor`, two
  launches, bit-identical to Pillow's Lanczos and the reference's fp32 lines :330-338).  The 9 x 3 patch PNGs per sample
  (:283-327) are NEVER opened: `networks_detr` reads `bbox_patch` for its shape only (networks_detr.py:133-187), so 'patches' is
  a 0-stride zero view of the right shape; 'patches_orig' / 'patch_masks' / 'background_orig' (snapshot image grids only) are absent:
  the `images` snapshot kinds read their uint8 crops through `patch_crops(idx)` instead.
  `LayoutDataset.collate` keeps the pages uint8 and the patch placeholder 0-stride (torch's default collate would materialise 7 MB
  of zeros per sample); `training_loop()` passes it to the DataLoader and calls `batch_backgrounds_to_device`.
* mode='raw' (opt-in; `LDETR_DATASET_MODE=raw`, `python -m layoutdetr_amd.dropin --dataset-mode=raw`): as 'device' in every key except
  'background', which is the page's PNG FILE BYTES (`RawPage`: the zip entries are ZIP_STORED, a read) when `scan_png` finds the file
  eligible -- 8-bit RGB, not interlaced, a zlib stream of stored blocks only, which is what the reference's dataset_tool.py:325-363 writes
  (compress_level=0) -- and the Pillow-decoded uint8 page, exactly as 'device' produces it, otherwise (a per-item fallback, counted in
  `route_counts`).  `batch_backgrounds_to_device` decodes the raw pages of a batch on the GPU (`decode_pages`, csrc/png_decode.hip: a gather of
  the stored payload + PNG's row filters undone, bit-identical to Pillow) and proceeds as for 'device'.
* mode='packed' (opt-in; `LDETR_DATASET_MODE=packed`, `--dataset-mode=packed`): as 'raw', and a page whose file carries the encoder's ldIX index
  (`python -m layoutdetr_amd.repack_dataset`) also goes out as file bytes and is inflated on the GPU (csrc/png_inflate.hip);
  everything else is decoded with Pillow.  `route_counts` has a 'packed' key in this mode.  The inflate kernel's per-page status words are checked
  at the next `batch_backgrounds_to_device` call and at `close()`: no synchronisation point is added to the step.
* mode='reference': every key of the reference's item, computed on the host exactly as the reference does (PIL decode + Lanczos
  resize, float normalise, transpose) — what `setup_snapshot` (training_loop.py:36-59) needs, and the side that
  tests/golden/dataset.npz (the reference's own `__getitem__` on tests/golden/dataset_tiny.zip) pins.

Device side (`background_to_tensor`, `csrc/resample.hip`): there is no CPU fallback — without the HIP library or a GPU tensor it raises.
"""
import ctypes
import io
import json
import os
import struct
import zipfile
import zlib

import numpy as np
import torch

from ..hip import core
from ..pil_coeffs import FILTER_LANCZOS, coeff_table

RGB_MEAN = (0.485, 0.456, 0.406)   # dataset_layoutganpp.py:268
RGB_STD = (0.229, 0.224, 0.225)    # dataset_layoutganpp.py:269

_coeff_cache = {}


def resample_coeffs(in_size, out_size, device):
    """(bounds [out, 2] int32, weights [ksize, out] int32, ksize) of Pillow's Lanczos window on `device`: the host table of
    pil_coeffs.coeff_table, uploaded once per (in, out, device)."""
    key = (int(in_size), int(out_size), str(device))
    hit = _coeff_cache.get(key)
    if hit is not None:
        return hit
    bounds, weights, ksize = coeff_table(in_size, out_size, FILTER_LANCZOS)
    out = (torch.tensor(bounds, device=device), torch.tensor(weights, device=device), ksize)     # copies: the host table is shared
    _coeff_cache[key] = out
    return out


PAGE_FILTER_TILE = 64                                   # csrc/page_filter.hip PF_TILE: one block per 64 x 64 output tile
PAGE_FILTER_KINDS = {'blur': 1, 'edge': 2}              # include/ldetr_hip.h LDETR_PAGE_FILTER_*


def filter_pages(pages_u8, kind, radius=3.0):
    """The page filters of the reference's generate.py --bg-preprocessing on decoded pages, uint8 [n, H, W, 3] (or [H, W, 3]) in GPU memory ->
    a new tensor of the same shape, one launch for all pages (csrc/page_filter.hip), bit-identical to Pillow:
    'blur' = ImageFilter.GaussianBlur(radius), 0 < radius <= 5 (generate.py:268); 'edge' = convert('L').filter(FIND_EDGES).convert('RGB') (:281)."""
    core.require_gpu(pages_u8)
    if kind not in PAGE_FILTER_KINDS:
        raise ValueError(f'filter_pages: unknown kind {kind!r}: one of {sorted(PAGE_FILTER_KINDS)}')
    if pages_u8.dtype != torch.uint8 or pages_u8.ndim not in (3, 4) or pages_u8.shape[-1] != 3 or 0 in pages_u8.shape[-3:]:
        raise ValueError(f'filter_pages: expected uint8 [n, H, W, 3] or [H, W, 3] (got {pages_u8.dtype} {tuple(pages_u8.shape)})')
    radius = float(radius)
    if kind == 'blur' and not 0.0 < radius <= 5.0:
        raise ValueError(f'filter_pages: blur radius must be in (0, 5] (got {radius})')
    src = pages_u8.contiguous()
    if src.data_ptr() % 4:                              # a view that starts in the middle of a buffer: the kernel loads 4 bytes at a time
        src = src.clone()
    out = torch.empty_like(src)
    n = src.shape[0] if src.ndim == 4 else 1
    H, W = src.shape[-3], src.shape[-2]
    core.check(core.lib().ldetr_page_filter_u8(core.ptr(src), core.ptr(out), n, H, W, PAGE_FILTER_KINDS[kind], radius, core.stream()), 'page_filter_u8')
    return out


def background_to_tensor(pages_u8, background_size, return_u8=False, mean=RGB_MEAN, std=RGB_STD, page_filter=None):
    """Decoded pages, uint8 [n, H, W, 3] (or [H, W, 3]) in GPU memory -> float32 [n, 3, S, S]: what `_load_raw_data` returns under
    'background', for the whole batch in two launches.  return_u8 additionally returns the resized uint8 pages [n, S, S, 3].
    page_filter ('blur' / 'edge'; None: nothing changes) runs `filter_pages` on the pages before the resize, as generate.py:267-269, 280-282."""
    core.require_gpu(pages_u8)
    if page_filter is not None and page_filter not in PAGE_FILTER_KINDS:
        raise ValueError(f'background_to_tensor: page_filter must be None or one of {sorted(PAGE_FILTER_KINDS)} (got {page_filter!r})')
    single = pages_u8.ndim == 3
    if single:
        pages_u8 = pages_u8[None]
    if pages_u8.dtype != torch.uint8 or pages_u8.ndim != 4 or pages_u8.shape[-1] != 3:
        raise ValueError('background_to_tensor: expected uint8 [n, H, W, 3] (the reference asserts 3 channels, dataset_layoutganpp.py:334)')
    pages_u8 = pages_u8.contiguous() if page_filter is None else filter_pages(pages_u8, page_filter)
    n, H, W, _ = pages_u8.shape
    S = int(background_size)
    dev = pages_u8.device
    hb, hk, hks = resample_coeffs(W, S, dev)
    vb, vk, vks = resample_coeffs(H, S, dev)
    tmp = torch.empty((n, H, S, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
    u8 = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) if return_u8 else None
    m = [float(np.float32(v)) for v in mean]
    s = [float(np.float32(v)) for v in std]
    core.check(core.lib().ldetr_resize_normalize_u8(core.ptr(pages_u8), n, H, W, S, S, core.ptr(hb), core.ptr(hk), hks, core.ptr(vb), core.ptr(vk), vks,
                                                    core.ptr(tmp), core.ptr(u8) if u8 is not None else None, core.ptr(out),
                                                    m[0], m[1], m[2], s[0], s[1], s[2], core.stream()), 'resize_normalize_u8')
    if single:
        out = out[0]
        u8 = u8[0] if u8 is not None else None
    return (out, u8) if return_u8 else out


# ---------------------------------------------------------------------------------------------------------------------------------
# stored-block PNG pages: host scan + device decode (csrc/png_decode.hip)

DATASET_MODES = ('device', 'raw', 'packed', 'reference')
PNG_NOT_ELIGIBLE, PNG_MALFORMED = 3, 4                  # include/ldetr_hip.h LDETR_PNG_*
PNG_INFLATE_ERRORS = {1: 'an invalid Huffman code or block header', 2: 'a sub-block that does not yield its 512 bytes or does not end at the next index entry',
                      4: 'a block header that does not end at index entry 0', 8: 'a distance before the segment start', 16: 'no end-of-block code or empty stored block',
                      32: 'a filter byte that differs from the index', 64: 'matches left unresolved', 128: 'a stale segment table'}      # LDETR_PNG_INFLATE_*


def default_dataset_mode():
    """The mode a `LayoutDataset` built without an explicit `mode` takes: LDETR_DATASET_MODE (set by `dropin --dataset-mode`), else 'device'."""
    mode = os.environ.get('LDETR_DATASET_MODE') or 'device'
    if mode not in DATASET_MODES:
        raise ValueError(f'LDETR_DATASET_MODE={mode!r}: one of {DATASET_MODES}')
    return mode


class RawPage:
    """One eligible page PNG as `scan_png` found it: `data` the file bytes (1-D uint8, numpy or a CPU torch tensor), `width`, `height`,
    `segments` int64 [k, 3] = (offset in file, offset in the filtered scanline stream, length) and `row_starts` int32 [r], the rows at
    which `decode_pages` starts an independent row range.  `kind` is 'stored' (the above) or 'packed': an indexed file of compressed blocks
    (DESIGN.md §18), whose `packed` = (int64 [k, 4] = (offset of the IDAT data, bytes, block type, first index entry), offset of the ldIX data) replaces
    `segments` (None then)."""
    __slots__ = ('data', 'width', 'height', 'segments', 'row_starts', 'kind', 'packed')

    def __init__(self, data, width, height, segments, row_starts, kind='stored', packed=None):
        self.data, self.width, self.height, self.segments, self.row_starts = data, int(width), int(height), segments, row_starts
        if kind not in ('stored', 'packed') or (kind == 'packed') != (packed is not None):
            raise ValueError("RawPage: kind is 'stored', or 'packed' with its segment table")
        self.kind, self.packed = kind, packed

    shape = property(lambda self: (self.height, self.width, 3))          # of the decoded page

    def tensor(self):
        return self.data if torch.is_tensor(self.data) else torch.from_numpy(self.data)

    def pin_memory(self, device=None):
        """What DataLoader(pin_memory=True) calls on a batch element: the file bytes in page-locked memory, the tables as they are."""
        return RawPage(self.tensor().pin_memory(), self.width, self.height, self.segments, self.row_starts, self.kind, self.packed)


def _verify_png(data):
    """Chunk CRC-32s and the zlib stream's Adler-32 of a file `ldetr_png_scan` accepted, as Pillow checks them."""
    buf = data.tobytes()
    pos, idat = 8, []
    while pos + 12 <= len(buf):
        n, = struct.unpack('>I', buf[pos:pos + 4])
        crc, = struct.unpack('>I', buf[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(buf[pos + 4:pos + 8 + n]) != crc:
            raise ValueError(f'scan_png: chunk {buf[pos + 4:pos + 8]!r} at byte {pos}: CRC-32 mismatch')
        if buf[pos + 4:pos + 8] == b'IDAT':
            idat.append(buf[pos + 8:pos + 8 + n])
        if buf[pos + 4:pos + 8] == b'IEND':
            break
        pos += 12 + n
    return b''.join(idat)


def _scan_png_packed(arr, verify):
    """`ldetr_png_scan_packed` on a file the stored scan did not take -> a 'packed' `RawPage`, or None."""
    from .. import _lib
    lib = _lib.load()
    w, h = ctypes.c_int(0), ctypes.c_int(0)
    k, r, ix = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    src = arr.ctypes.data_as(ctypes.c_void_p)

    def call(seg, rows):
        rc = lib.ldetr_png_scan_packed(src, arr.size, ctypes.byref(w), ctypes.byref(h), seg.ctypes.data_as(ctypes.c_void_p) if seg is not None else None,
                                       len(seg) if seg is not None else 0, ctypes.byref(k), ctypes.byref(ix), rows.ctypes.data_as(ctypes.c_void_p) if rows is not None else None,
                                       len(rows) if rows is not None else 0, ctypes.byref(r))
        if rc == PNG_MALFORMED:
            raise ValueError(lib.ldetr_last_error().decode('utf-8', 'replace'))
        if rc != PNG_NOT_ELIGIBLE:
            _lib.check(rc, 'png_scan_packed')
        return rc
    if call(None, None) == PNG_NOT_ELIGIBLE:
        return None
    seg, rows = np.zeros((k.value, 4), np.int64), np.zeros(r.value, np.int32)
    call(seg, rows)
    if verify:
        try:
            zlib.decompress(_verify_png(arr))                              # (raises on a wrong Adler-32)
        except zlib.error as e:
            raise ValueError(f'scan_png: the zlib stream does not check out ({e})')
    return RawPage(arr, w.value, h.value, None, rows, 'packed', (seg, int(ix.value)))


def scan_png(data, verify=False, packed=False):
    """One PNG file (bytes, or a 1-D uint8 array) -> `RawPage` when the device path takes it, None when it is a well-formed PNG that it does
    not take (compressed blocks, interlace, palette, 16-bit, grey / RGBA, ...: the caller decodes those with Pillow); ValueError for a malformed
    file.  Host work only (`ldetr_png_scan`).  verify=True also checks every chunk's CRC-32 and the stream's Adler-32, which Pillow does and the
    scan does not, and raises ValueError on a mismatch.  packed=True: a file the stored scan does not take is offered to `ldetr_png_scan_packed`
    (the indexed files of `render.encode_png(index=True)`) before None is returned; the RawPage's `kind` tells the two apart."""
    # (bytes are copied once: torch takes writable arrays only; LayoutDataset reads the zip entry straight into an array instead)
    arr = np.frombuffer(data, np.uint8).copy() if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8).reshape(-1)
    from .. import _lib
    lib = _lib.load()                                    # (not core.lib(): that registers a GPU workspace, and this runs in DataLoader workers)
    w, h, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    k, r = ctypes.c_int64(0), ctypes.c_int64(0)
    src = arr.ctypes.data_as(ctypes.c_void_p)

    def call(seg, rows):
        rc = lib.ldetr_png_scan(src, arr.size, ctypes.byref(w), ctypes.byref(h), ctypes.byref(c), seg.ctypes.data_as(ctypes.c_void_p) if seg is not None else None,
                                len(seg) if seg is not None else 0, ctypes.byref(k), rows.ctypes.data_as(ctypes.c_void_p) if rows is not None else None,
                                len(rows) if rows is not None else 0, ctypes.byref(r))
        if rc == PNG_MALFORMED:
            raise ValueError(lib.ldetr_last_error().decode('utf-8', 'replace'))
        if rc != PNG_NOT_ELIGIBLE:
            _lib.check(rc, 'png_scan')
        return rc
    if call(None, None) == PNG_NOT_ELIGIBLE:
        return _scan_png_packed(arr, verify) if packed else None
    seg, rows = np.zeros((k.value, 3), np.int64), np.zeros(r.value, np.int32)
    call(seg, rows)
    if verify:
        z = _verify_png(arr)
        payload = b''.join(arr[o:o + n].tobytes() for o, _, n in seg)
        if len(z) < 4 or zlib.adler32(payload) != struct.unpack('>I', z[-4:])[0]:
            raise ValueError('scan_png: Adler-32 mismatch in the zlib stream')
    return RawPage(arr, w.value, h.value, seg, rows)


def _png_tables(pages):
    """Host tables of one `ldetr_png_decode_u8` call: file offsets (each file 16-byte aligned) [n + 1], segments [k, 4], row ranges [j, 3], buffer bytes."""
    off, segs, jobs, pos = [], [], [], 0
    for i, p in enumerate(pages):
        off.append(pos)
        pos += (int(p.tensor().numel()) + 15) // 16 * 16
        segs.append(np.concatenate([np.full((len(p.segments), 1), i, np.int64), np.asarray(p.segments, np.int64).reshape(-1, 3)], 1))
        starts = np.asarray(p.row_starts, np.int32).reshape(-1)
        jobs.append(np.stack([np.full(len(starts), i, np.int32), starts, np.append(starts[1:], np.int32(p.height))], 1))
    off.append(pos)                                                        # a multiple of 16: the end of the padded last file
    return np.asarray(off, np.int64), np.ascontiguousarray(np.concatenate(segs, 0)), np.ascontiguousarray(np.concatenate(jobs, 0).astype(np.int32)), pos


def _decode_group(pages, device, phases=3, state=None):
    """One `ldetr_png_decode_u8` call: RawPages of one size -> uint8 [n, H, W, 3] on `device`.  `state` (tools/bench_page_decode.py) keeps the
    uploaded buffers between calls that time the two launches apart."""
    from .. import _lib
    n, H, W = len(pages), pages[0].height, pages[0].width
    if state is None or 'files' not in state:
        off, seg, jobs, nbytes = _png_tables(pages)
        host = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=all(p.tensor().is_pinned() for p in pages))
        for i, p in enumerate(pages):
            t = p.tensor()
            host[int(off[i]):int(off[i]) + t.numel()] = t
        tables = torch.from_numpy(np.concatenate([off.view(np.uint8), seg.reshape(-1).view(np.uint8), jobs.reshape(-1).view(np.uint8)]))
        st = dict(off=off, seg=seg, jobs=jobs, files=host.to(device, non_blocking=True), tables=tables.to(device, non_blocking=True),
                  scratch=torch.empty((n * H * (1 + 3 * W) + 15) // 16 * 16, dtype=torch.uint8, device=device),
                  dst=torch.empty((n, H, W, 3), dtype=torch.uint8, device=device))
        if state is not None:
            state.update(st)
    else:
        st = state
    core.require_gpu(st['files'])
    tp = st['tables'].data_ptr()                                          # [file offsets | segments | row ranges], as on the host
    a = _lib.PngDecodeArgs(struct_bytes=ctypes.sizeof(_lib.PngDecodeArgs), n=n, H=H, W=W, phases=phases, reserved=0,
                           files=core.ptr(st['files']), files_bytes=st['files'].numel(),
                           file_off=st['off'].ctypes.data, file_off_dev=tp,
                           segments=st['seg'].ctypes.data, segments_dev=tp + st['off'].nbytes, n_segments=len(st['seg']),
                           jobs=st['jobs'].ctypes.data, jobs_dev=tp + st['off'].nbytes + st['seg'].nbytes, n_jobs=len(st['jobs']),
                           scratch=core.ptr(st['scratch']), scratch_bytes=st['scratch'].numel(), dst=core.ptr(st['dst']))
    core.check(core.lib().ldetr_png_decode_u8(ctypes.byref(a), core.stream()), 'png_decode_u8')
    return st['dst']


def _inflate_group(pages, device, phases=3, state=None):
    """One `ldetr_png_inflate_u8` call: 'packed' RawPages of one size -> (uint8 [n, H, W, 3], int32 [n] status) on `device`.  `state` as in `_decode_group`."""
    from .. import _lib
    n, H, W = len(pages), pages[0].height, pages[0].width
    if state is None or 'files' not in state:
        off, pos, jobs = [], 0, []
        for i, p in enumerate(pages):
            off.append(pos)
            pos += (int(p.tensor().numel()) + 15) // 16 * 16
            starts = np.asarray(p.row_starts, np.int32).reshape(-1)
            jobs.append(np.stack([np.full(len(starts), i, np.int32), starts, np.append(starts[1:], np.int32(p.height))], 1))
        off = np.asarray(off + [pos], np.int64)
        seg = np.ascontiguousarray(np.concatenate([np.asarray(p.packed[0], np.int64).reshape(-1, 4) for p in pages], 0))
        ix = np.asarray([p.packed[1] for p in pages], np.int64)
        jobs = np.ascontiguousarray(np.concatenate(jobs, 0).astype(np.int32))
        host = torch.zeros(pos, dtype=torch.uint8, pin_memory=all(p.tensor().is_pinned() for p in pages))
        for i, p in enumerate(pages):
            t = p.tensor()
            host[int(off[i]):int(off[i]) + t.numel()] = t
        tables = torch.from_numpy(np.concatenate([off.view(np.uint8), seg.reshape(-1).view(np.uint8), ix.view(np.uint8), jobs.reshape(-1).view(np.uint8)]))
        st = dict(off=off, seg=seg, ix=ix, jobs=jobs, files=host.to(device, non_blocking=True), tables=tables.to(device, non_blocking=True),
                  scratch=torch.empty((n * H * (1 + 3 * W) + 15) // 16 * 16, dtype=torch.uint8, device=device),
                  dst=torch.empty((n, H, W, 3), dtype=torch.uint8, device=device), status=torch.zeros(n, dtype=torch.int32, device=device))
        if state is not None:
            state.update(st)
    else:
        st = state
    core.require_gpu(st['files'])
    tp = st['tables'].data_ptr()                                          # [file offsets | segments | index offsets | row ranges], as on the host
    a = _lib.PngInflateArgs(struct_bytes=ctypes.sizeof(_lib.PngInflateArgs), n=n, H=H, W=W, phases=phases, reserved=0,
                            files=core.ptr(st['files']), files_bytes=st['files'].numel(),
                            file_off=st['off'].ctypes.data, file_off_dev=tp,
                            segments=st['seg'].ctypes.data, segments_dev=tp + st['off'].nbytes,
                            index_off=st['ix'].ctypes.data, index_off_dev=tp + st['off'].nbytes + st['seg'].nbytes,
                            jobs=st['jobs'].ctypes.data, jobs_dev=tp + st['off'].nbytes + st['seg'].nbytes + st['ix'].nbytes, n_jobs=len(st['jobs']),
                            scratch=core.ptr(st['scratch']), scratch_bytes=st['scratch'].numel(), dst=core.ptr(st['dst']), status=core.ptr(st['status']))
    core.check(core.lib().ldetr_png_inflate_u8(ctypes.byref(a), core.stream()), 'png_inflate_u8')
    return st['dst'], st['status']


class PageStatus(object):
    """The status words of the 'packed' groups of one `decode_pages` call, on their way to the host: `check()` waits for the copy (not for anything
    enqueued after it) and raises ValueError naming the first page whose file the inflate kernel found corrupt."""

    def __init__(self):
        self.parts = []                                                    # (pinned int32 [n], positions in the call's page list)
        self.event = None

    def add(self, status, positions):
        host = torch.empty(status.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(status, non_blocking=True)
        self.parts.append((host, list(positions)))
        self.event = torch.cuda.Event()
        self.event.record()

    def tensor(self):
        """int32 [pages of packed groups], in group order."""
        if self.event is not None:
            self.event.synchronize()
        return torch.cat([h for h, _ in self.parts]) if self.parts else torch.zeros(0, dtype=torch.int32)

    def check(self, names=None):
        if self.event is not None:
            self.event.synchronize()
        for host, positions in self.parts:
            for v, i in zip(host.tolist(), positions):
                if v:
                    what = '; '.join(t for b, t in PNG_INFLATE_ERRORS.items() if v & b)
                    raise ValueError(f'decode_pages: page {names[i] if names else i}: the indexed PNG is corrupt (status {v}: {what})')


def decode_pages(raw_pages, device, status=None):
    """`RawPage`s -> the decoded pages in GPU memory, bit-identical to np.array(PIL.Image.open(...)): uint8 [n, H, W, 3] when the pages share
    a size, else a list of [H, W, 3] tensors in the order given.  One `ldetr_png_decode_u8` call ('stored' pages) or `ldetr_png_inflate_u8` call
    ('packed' pages; two launches either way) per distinct kind and page size.  The inflate kernel reports a corrupt file in a status word per page:
    with status=None the call waits for them and raises ValueError naming the page; pass a `PageStatus` to collect them instead and `check()` it later
    (`batch_backgrounds_to_device` does, so that the training step gets no synchronisation point).  A page's word is written with plain stores by
    every workgroup (segment) that found an error, so it holds the bits of ONE of them, not their union: non-zero always means corrupt, but the
    message may name only some of the faults of a file that has several.
    There is no CPU path: without a GPU device it raises."""
    raw_pages = list(raw_pages)
    if not raw_pages or not all(isinstance(p, RawPage) for p in raw_pages):
        raise ValueError('decode_pages: expected a non-empty sequence of RawPage')
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f'decode_pages: needs a GPU device (got {device}); layoutdetr_amd has no CPU path')
    groups = {}
    for i, p in enumerate(raw_pages):
        groups.setdefault((p.kind, p.height, p.width), []).append(i)
    collect = PageStatus() if status is None else status

    def run(idx):
        pages = [raw_pages[i] for i in idx]
        if pages[0].kind == 'stored':
            return _decode_group(pages, device)
        dec, st = _inflate_group(pages, device)
        collect.add(st, idx)
        return dec
    if len(groups) == 1:
        out = run(list(range(len(raw_pages))))
    else:
        out = [None] * len(raw_pages)
        for idx in groups.values():
            dec = run(idx)
            for j, i in enumerate(idx):
                out[i] = dec[j]
    if status is None:
        collect.check()
    return out


# batch_backgrounds_to_device: the PageStatus of the call before.  ONE list per process, not per dataset: the function sees a collated batch, not the
# dataset it came from, and a training process decodes the pages of one training set.  So the error of a corrupt page surfaces at the next
# batch_backgrounds_to_device call whichever dataset's batch that is, or when a mode='packed' dataset is closed (datasets of other modes do not look).
_pending_status = []


def check_pending_status():
    """Raise for a corrupt indexed page the previous `batch_backgrounds_to_device` call decoded (its status words crossed to the host since).
    Process-wide: see `_pending_status`."""
    while _pending_status:
        _pending_status.pop(0).check()


# ---------------------------------------------------------------------------------------------------------------------------------
# host side: the zip + non_image.json reader


def to_dense_batch(data, is_str=False):
    """dataset_layoutganpp.py:29-41: pad the leading (element) axis to nine slots; mask = which slots hold an element."""
    n = len(data)
    if n > 9:
        raise ValueError(f'to_dense_batch: {n} elements, the format holds at most 9 per layout')
    mask = np.arange(9) < n
    if is_str:
        return list(data) + [''] * (9 - n), mask
    data = np.asarray(data)
    out = np.zeros((9,) + data.shape[1:], dtype=data.dtype)
    out[:n] = data
    return out, mask


def _patch_canvas_size(width, height):
    """(:287-292) the longer side becomes 256, the other keeps the aspect ratio, rounded down to an even number."""
    if width > height:
        return 256, int(float(height) / float(width) * 256.0) // 2 * 2
    return int(float(width) / float(height) * 256.0) // 2 * 2, 256


class Dataset(torch.utils.data.Dataset):
    """Base class with the reference's constructor arguments and properties (dataset_layoutganpp.py:45-210)."""

    def __init__(self, name, raw_shape, num_bbox_labels, max_size=None, use_labels=False, background_size=1024, random_seed=0):
        self._name = name
        self._raw_shape = list(raw_shape)
        self._num_bbox_labels = num_bbox_labels
        self._colors = None
        self._use_labels = use_labels
        self.background_size = background_size
        self._raw_labels = None
        self._label_shape = None
        self._raw_idx = np.arange(self._raw_shape[0], dtype=np.int64)
        if (max_size is not None) and (self._raw_idx.size > max_size):       # :66-69: a seeded subset, kept in file order
            np.random.RandomState(random_seed).shuffle(self._raw_idx)
            self._raw_idx = np.sort(self._raw_idx[:max_size])

    def _get_raw_labels(self):
        if self._raw_labels is None:
            self._raw_labels = self._load_raw_labels() if self._use_labels else None
            if self._raw_labels is None:
                self._raw_labels = np.zeros([self._raw_shape[0], 0], dtype=np.float32)
            assert isinstance(self._raw_labels, np.ndarray) and self._raw_labels.shape[0] == self._raw_shape[0]
            assert self._raw_labels.dtype in [np.float32, np.int64]
            if self._raw_labels.dtype == np.int64:
                assert self._raw_labels.ndim == 1 and np.all(self._raw_labels >= 0)
        return self._raw_labels

    def close(self):
        pass

    def _load_raw_data(self, raw_idx):
        raise NotImplementedError

    def _load_raw_labels(self):
        raise NotImplementedError

    def __getstate__(self):
        return dict(self.__dict__, _raw_labels=None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self._raw_idx.size

    def __getitem__(self, idx):
        return self._load_raw_data(self._raw_idx[idx]), self.get_label(idx)

    def get_label(self, idx):
        label = self._get_raw_labels()[self._raw_idx[idx]]
        if label.dtype == np.int64:
            onehot = np.zeros(self.label_shape, dtype=np.float32)
            onehot[label] = 1
            label = onehot
        return label.copy()

    def get_details(self, idx):
        raw_idx = int(self._raw_idx[idx])
        return dict(raw_idx=raw_idx, raw_label=self._get_raw_labels()[raw_idx].copy())

    name = property(lambda self: self._name)
    patch_shape = property(lambda self: list(self._raw_shape[1:]))
    num_assets = property(lambda self: self.patch_shape[0])
    num_channels = property(lambda self: self.patch_shape[1])
    height = property(lambda self: self.patch_shape[2])
    width = property(lambda self: self.patch_shape[3])
    background_size_for_training = property(lambda self: self.background_size)
    num_bbox_labels = property(lambda self: self._num_bbox_labels)

    @property
    def colors(self):
        """One RGB triple per bbox label for the snapshot grids (:183-188 takes them from seaborn's 'husl' palette; seaborn is not a
        dependency of the hot path: evenly spaced hues at fixed lightness / saturation instead — drawing only, never a network input)."""
        if self._colors is None:
            import colorsys
            n = self._num_bbox_labels
            self._colors = [tuple(int(v * 255) for v in colorsys.hls_to_rgb(i / max(n, 1), 0.65, 0.9)) for i in range(n)]
        return self._colors

    @property
    def label_shape(self):
        if self._label_shape is None:
            raw = self._get_raw_labels()
            self._label_shape = [int(np.max(raw)) + 1] if raw.dtype == np.int64 else raw.shape[1:]
        return list(self._label_shape)

    @property
    def label_dim(self):
        assert len(self.label_shape) == 1
        return self.label_shape[0]

    has_labels = property(lambda self: any(x != 0 for x in self.label_shape))
    has_onehot_labels = property(lambda self: self._get_raw_labels().dtype == np.int64)


class LayoutDataset(Dataset):
    """dataset_layoutganpp.py:214-352.  See the module docstring for `mode`."""

    def __init__(self, path, xflip=False, background_size=1024, mode=None, verify_png=False, **super_kwargs):
        if mode is None:
            mode = default_dataset_mode()
        if mode not in DATASET_MODES:
            raise ValueError("LayoutDataset: mode must be 'device', 'raw', 'packed' or 'reference'")
        self.verify_png = bool(verify_png)
        self.route_counts = {'raw': 0, 'decoded': 0}         # mode='raw': items whose page went out as file bytes / was decoded here with Pillow
        if mode == 'packed':                                 # ... / went out as the bytes of an indexed file of compressed blocks
            self.route_counts = {'raw': 0, 'packed': 0, 'decoded': 0}
        self._path = path
        self.background_size = background_size
        self.mode = mode
        self._zipfile = None
        self._rawfile = None                                 # mode='raw': a second handle on the archive for reading stored entries as they are
        if os.path.splitext(self._path)[1].lower() != '.zip':
            raise IOError('Path must point to a zip')                        # :229
        self._type = 'zip'
        self._all_fnames = set(self._get_zipfile().namelist())
        if 'non_image.json' not in self._all_fnames:
            raise IOError(f'{path}: no non_image.json in the archive')
        with self._open_file('non_image.json') as f:
            self._samples = json.load(f)['samples']
        if not self._samples:
            raise IOError(f'{path}: non_image.json lists no samples')
        parts = self._path.split('/')
        name = parts[-3] if len(parts) >= 3 else os.path.splitext(os.path.basename(self._path))[0]      # :237
        raw_shape = [len(self._samples)] + self._patch_orig_shape(0)
        num_bbox_labels = self._samples[0][1]['attr']['num_bbox_labels']
        super().__init__(name=name, raw_shape=raw_shape, num_bbox_labels=num_bbox_labels, background_size=background_size, **super_kwargs)

    def _get_zipfile(self):
        if self._zipfile is None:
            self._zipfile = zipfile.ZipFile(self._path)
        return self._zipfile

    def _open_file(self, fname):
        return self._get_zipfile().open(fname, 'r')

    def _read_entry(self, fname):
        """The bytes of one archive entry as a writable uint8 array.  A ZIP_STORED entry (what dataset_tool.py writes) is read straight from the
        archive file at its data offset: no inflate, and not zipfile's CRC-32 pass over the bytes either (`scan_png(verify=True)` checks the PNG's own
        checksums); any other entry goes through zipfile."""
        info = self._get_zipfile().getinfo(fname)
        if info.compress_type != zipfile.ZIP_STORED or info.flag_bits & 0x1:
            return np.frombuffer(self._get_zipfile().read(fname), np.uint8).copy()
        if self._rawfile is None:
            self._rawfile = open(self._path, 'rb')
        f = self._rawfile
        f.seek(info.header_offset)
        hdr = f.read(30)
        if len(hdr) != 30 or hdr[:4] != b'PK\x03\x04':
            raise IOError(f'{self._path}: no local file header for {fname}')
        n, m = struct.unpack('<HH', hdr[26:30])
        f.seek(info.header_offset + 30 + n + m)
        data = np.empty(info.file_size, np.uint8)
        if f.readinto(data) != data.size:
            raise IOError(f'{self._path}: {fname}: short read')
        return data

    def close(self):
        try:
            if self.mode == 'packed':                        # the status words of the last batch decoded on the device (no other mode produces any)
                check_pending_status()
        finally:
            self._close_files()

    def _close_files(self):
        try:
            if self._zipfile is not None:
                self._zipfile.close()
            if self._rawfile is not None:
                self._rawfile.close()
        finally:
            self._zipfile = self._rawfile = None

    def __getstate__(self):                      # DataLoader workers re-open the archive themselves
        return dict(super().__getstate__(), _zipfile=None, _rawfile=None)

    def _patch_orig_shape(self, raw_idx):
        """[9, 3, H, W] of sample `raw_idx`'s '<base>_0_patch_orig.png' — the reference decodes the whole sample to learn this (:238);
        the PNG header is enough."""
        import PIL.Image
        base = self._samples[raw_idx][0]
        with self._open_file(base + '_0_patch_orig.png') as f:
            im = PIL.Image.open(f)
            w, h = im.size
        return [9, 3, h, w]

    def _decode(self, fname):
        import PIL.Image
        with self._open_file(fname) as f:
            im = PIL.Image.open(f)
            im.load()
        return im

    def _fields(self, raw_idx):
        """The non-image fields of one sample (:270-281), padded to nine slots."""
        meta = self._samples[raw_idx][1]
        bboxes = np.array(meta['bboxes'])
        bboxes_batch, mask = to_dense_batch(bboxes.reshape(-1, 4) if bboxes.size else np.zeros((0, 4)))
        labels_batch, _ = to_dense_batch(np.array(meta['labels']))
        texts_batch, _ = to_dense_batch(meta['texts'], is_str=True)
        return dict(name=meta['attr']['name'], W_page=meta['attr']['width'], H_page=meta['attr']['height'],
                    bboxes=bboxes_batch.astype(np.float32), labels=labels_batch.astype(np.int64), texts=texts_batch, mask=mask), int(mask.sum())

    def layouts(self):
        """The layouts of all items without their images: bboxes [n, 9, 4] float32, labels [n, 9] int64, mask [n, 9] bool (True = a real
        element) as torch tensors, in item order (max_size honoured).  Reads non_image.json's fields only; no PNG is decoded."""
        fields = [self._fields(int(i))[0] for i in self._raw_idx]
        return (torch.from_numpy(np.stack([f['bboxes'] for f in fields]).astype(np.float32)),
                torch.from_numpy(np.stack([f['labels'] for f in fields]).astype(np.int64)),
                torch.from_numpy(np.stack([f['mask'] for f in fields]).astype(np.bool_)))

    def patch_crops(self, idx):
        """The uint8 text patches of item `idx` as the `images` snapshot kinds paste them (util.py:159-163; DESIGN.md §13 rule 8): per slot the
        centre width x height window of '<base>_<k>_patch_orig.png', width = int(bbox[2] * W_page), height = int(bbox[3] * H_page) (fp32 products,
        truncated), or None for a padding slot and for a window that is empty or leaves the canvas (the reference would wrap or fail).  Works in
        either mode; only this item's patch files are decoded, and `__getitem__` is untouched."""
        raw_idx = int(self._raw_idx[idx])
        fields, n = self._fields(raw_idx)
        base = self._samples[raw_idx][0]
        W, H = np.float32(fields['W_page']), np.float32(fields['H_page'])
        out = [None] * len(fields['mask'])
        for k in range(n):
            b = fields['bboxes'][k].astype(np.float32)
            with np.errstate(all='ignore'):
                fw, fh = b[2] * W, b[3] * H
            if not (np.isfinite(fw) and np.isfinite(fh)):
                continue
            width, height = int(fw), int(fh)
            po = np.array(self._decode(base + '_%d_patch_orig.png' % k))
            if po.ndim != 3 or po.shape[2] != 3:
                raise ValueError(f'{base}_{k}_patch_orig.png: expected an RGB patch (:305-315)')
            cy, cx = po.shape[0] // 2, po.shape[1] // 2
            y0, y1, x0, x1 = cy - height // 2, cy + height - height // 2, cx - width // 2, cx + width - width // 2
            if width < 1 or height < 1 or y0 < 0 or x0 < 0 or y1 > po.shape[0] or x1 > po.shape[1]:
                continue
            out[k] = np.ascontiguousarray(po[y0:y1, x0:x1])
        return out

    def _load_raw_data(self, raw_idx):
        raw_idx = int(raw_idx)
        out, n = self._fields(raw_idx)
        base = self._samples[raw_idx][0]
        if self.mode == 'device':
            page = np.array(self._decode(base + '_background_orig.png'))
            if page.ndim != 3 or page.shape[2] != 3:
                raise ValueError(f'{base}_background_orig.png: expected an RGB page (:334)')
            out['background'] = page                                                          # uint8 [H, W, 3]; resized + normalised on the GPU
            out['patches'] = np.broadcast_to(np.zeros((), np.float32), (9, 3, 256, 256))      # shape only, never read
            return out
        if self.mode in ('raw', 'packed'):
            data = self._read_entry(base + '_background_orig.png')
            raw = scan_png(data, verify=self.verify_png, packed=self.mode == 'packed')
            if raw is None:                                                                   # neither a stored-block nor (mode='packed') an indexed 8-bit RGB file: this item takes the 'device' route
                import PIL.Image
                page = np.array(PIL.Image.open(io.BytesIO(data.tobytes())))
                if page.ndim != 3 or page.shape[2] != 3:
                    raise ValueError(f'{base}_background_orig.png: expected an RGB page (:334)')
                raw = page
            self.route_counts[('packed' if raw.kind == 'packed' else 'raw') if isinstance(raw, RawPage) else 'decoded'] += 1
            out['background'] = raw
            out['patches'] = np.broadcast_to(np.zeros((), np.float32), (9, 3, 256, 256))
            return out
        import PIL.Image
        lanczos = PIL.Image.LANCZOS                                                           # = the reference's PIL.Image.ANTIALIAS (alias removed in Pillow 10)
        mean = np.reshape(np.array(RGB_MEAN).astype(np.float32), (1, 1, 3))
        std = np.reshape(np.array(RGB_STD).astype(np.float32), (1, 1, 3))

        def norm_chw(a):
            return ((a.astype(np.float32) / 255.0 - mean) / std).transpose(2, 0, 1)

        patches, patches_orig, patch_masks = [], [], []
        for i in range(n):
            im = self._decode(base + '_%d_patch.png' % i)                                    # :283-303
            wn, hn = _patch_canvas_size(im.width, im.height)
            small = np.array(im.resize((wn, hn), lanczos))
            assert small.ndim == 3 and small.shape[2] == 3
            canvas = np.zeros((256, 256, 3), np.float32)
            canvas[128 - hn // 2:128 + hn // 2, 128 - wn // 2:128 + wn // 2] = (small.astype(np.float32) / 255.0 - mean) / std
            patches.append(canvas.transpose(2, 0, 1))
            po = np.array(self._decode(base + '_%d_patch_orig.png' % i))                     # :305-315
            assert po.ndim == 3 and po.shape[2] == 3
            patches_orig.append(norm_chw(po))
            pm = np.array(self._decode(base + '_%d_patch_mask.png' % i))[:, :, np.newaxis]   # :317-327
            patch_masks.append((pm.astype(np.float32) / 255.0).transpose(2, 0, 1))
        out['patches'] = to_dense_batch(np.stack(patches, axis=0))[0]
        out['patches_orig'] = to_dense_batch(np.stack(patches_orig, axis=0))[0]
        out['patch_masks'] = to_dense_batch(np.stack(patch_masks, axis=0))[0]
        page = self._decode(base + '_background_orig.png')                                   # :329-340
        small = np.array(page.resize((self.background_size, self.background_size), lanczos))
        assert small.ndim == 3 and small.shape[2] == 3
        out['background'] = norm_chw(small)
        out['background_orig'] = norm_chw(np.array(page))
        return out

    def _load_raw_labels(self):
        """:344-352: the reference collects `page_label` and then returns None on every path (the conversion lines are commented out),
        so `use_labels=True` still yields a zero-width label: c_dim = 0 in every run `train.py` configures."""
        return None

    @staticmethod
    def collate(items):
        """DataLoader collate for mode='device' items: numeric fields stacked as torch's default collate does, 'texts' transposed to
        nine lists of B strings (what the default collate makes of a list of strings per item; training_loop.py:259 transposes it back),
        backgrounds kept uint8 — one [B, H, W, 3] tensor when the pages share a size, else a list — and 'patches' a 0-stride view."""
        samples, labels = zip(*items)
        b = len(samples)
        out = {}
        for k in ('bboxes', 'labels', 'mask'):
            out[k] = torch.from_numpy(np.stack([s[k] for s in samples], axis=0))
        for k in ('W_page', 'H_page'):
            out[k] = torch.tensor([s[k] for s in samples])
        out['name'] = [s['name'] for s in samples]
        out['texts'] = [tuple(s['texts'][j] for s in samples) for j in range(9)]
        pages = [s['background'] for s in samples]
        if any(isinstance(p, RawPage) for p in pages):                       # mode='raw': a list, file bytes and (fallback) decoded pages side by side
            out['background'] = [p if isinstance(p, RawPage) else torch.from_numpy(np.ascontiguousarray(p)) for p in pages]
        elif pages[0].dtype == np.uint8:
            same = all(p.shape == pages[0].shape for p in pages)
            out['background'] = torch.from_numpy(np.stack(pages, 0)) if same else [torch.from_numpy(np.ascontiguousarray(p)) for p in pages]
        else:
            out['background'] = torch.from_numpy(np.stack(pages, 0))
        p0 = samples[0]['patches']
        if 0 in p0.strides:
            out['patches'] = torch.zeros((1,) * (p0.ndim + 1)).expand(b, *p0.shape)
        else:
            out['patches'] = torch.from_numpy(np.stack([s['patches'] for s in samples], 0))
        for k in ('patches_orig', 'patch_masks', 'background_orig'):
            if k in samples[0]:
                out[k] = torch.from_numpy(np.stack([s[k] for s in samples], 0))
        return out, torch.from_numpy(np.stack(labels, 0))


def batch_backgrounds_to_device(background, background_size, device, page_filter=None):
    """'background' of a collated batch -> float32 [B, 3, S, S] on `device`.  uint8 pages (mode='device': one [B, H, W, 3] tensor, or a
    list when page sizes differ) are uploaded as bytes and resized + normalised by `background_to_tensor`, one call per distinct page
    size; float input (mode='reference' / other datasets) is what the reference already hands over (training_loop.py:264).
    `RawPage`s in the list (mode='raw') are uploaded as file bytes and decoded on the device first (`decode_pages`), then treated like the rest.
    page_filter ('blur' / 'edge') filters the uint8 pages before the resize; float backgrounds are already resized, so a filter on them raises."""
    if page_filter is not None and page_filter not in PAGE_FILTER_KINDS:
        raise ValueError(f'batch_backgrounds_to_device: page_filter must be None or one of {sorted(PAGE_FILTER_KINDS)} (got {page_filter!r})')
    check_pending_status()                                                   # mode='packed': what the call before found, by now on the host
    if torch.is_tensor(background):
        if background.dtype != torch.uint8:
            if page_filter is not None:
                raise ValueError('batch_backgrounds_to_device: page_filter needs the decoded uint8 pages (dataset mode=\'device\'), not float backgrounds')
            return background.to(device).float()
        return background_to_tensor(background.to(device, non_blocking=True), background_size, page_filter=page_filter)
    raw = [i for i, p in enumerate(background) if isinstance(p, RawPage)]
    if raw:                                                                  # mode='raw' / 'packed': the file bytes go up, the pages are decoded there
        status = PageStatus()
        dec = decode_pages([background[i] for i in raw], device, status=status)
        if status.parts:
            _pending_status.append(status)
        if len(raw) == len(background) and torch.is_tensor(dec):
            return background_to_tensor(dec, background_size, page_filter=page_filter)
        background = list(background)
        for j, i in enumerate(raw):
            background[i] = dec[j]
    groups = {}
    for i, p in enumerate(background):
        groups.setdefault(tuple(p.shape), []).append(i)
    out = torch.empty((len(background), 3, background_size, background_size), dtype=torch.float32, device=device)
    for idx in groups.values():
        pages = [background[i] for i in idx]
        pages = torch.stack([p.to(device, non_blocking=True) for p in pages]) if raw else torch.stack(pages).to(device, non_blocking=True)
        out[torch.tensor(idx, device=device)] = background_to_tensor(pages, background_size, page_filter=page_filter)
    return out


def patch_placeholder_to_device(patches, device):
    """'patches' of a collated batch on `device` without materialising a 0-stride placeholder (`.to()` would: 7 MB per sample)."""
    if patches.stride(0) == 0:
        return torch.zeros((1,) * patches.ndim, dtype=patches.dtype, device=device).expand(patches.shape)
    return patches.to(device)
