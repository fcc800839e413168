"""Numpy restatement of the snapshot-grid rendering rule (the reference's util.py:85-141), shared by test_snapshot_cpu.py,
test_snapshot_gpu.py and tools/gen_snapshot_golden.py.  Independent of the package: nothing here imports layoutdetr_amd.

Rules 1-3 (draw order, corners, pixel updates) restate what the reference's ImageDraw.rectangle calls do for boxes at least 3 page pixels wide
and high, and DEFINE the result for thinner / degenerate boxes; rules 4-6 restate PIL's BILINEAR resize and expand2square; rule 7 restates
torchvision's make_grid(padding=2, pad_value=0)."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def bilinear_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc with the triangle window: (bounds [out, 2], kk [out, ksize], ksize)."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(xmax):
            v = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - v if v < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            f = v * (1 << PRECISION_BITS)
            kk[xx, x] = int(-0.5 + f) if v < 0 else int(0.5 + f)
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def _pass(img, out_size, axis):
    in_size = img.shape[axis]
    if in_size == out_size:
        return img
    bounds, kk, _ = bilinear_coeffs(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, xmax = bounds[xx]
        acc = np.tensordot(kk[xx, :xmax].astype(np.int64), src[xmin:xmin + xmax], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_bilinear_u8(img, out_h, out_w):
    """Rule 5: horizontal pass into a uint8 intermediate, then the vertical pass."""
    return _pass(_pass(img, out_w, 1), out_h, 0)


def _trunc_i32(f):
    return int(min(max(math.trunc(float(f)), I32_MIN), I32_MAX)) if math.isfinite(float(f)) else (I32_MAX if f > 0 else I32_MIN)


def draw(bbox, valid, labels, colors, W, H, page=None):
    """Rules 1-3 -> uint8 [H, W, 3]."""
    img = np.full((H, W, 3), 255, np.uint8) if page is None else np.array(page, np.uint8).copy()
    assert img.shape == (H, W, 3)
    bbox = np.asarray(bbox, np.float32)
    two, fw, fh = np.float32(2), np.float32(W), np.float32(H)
    todo = []
    with np.errstate(all='ignore'):
        for i in range(bbox.shape[0]):
            if not valid[i]:
                continue
            xc, yc, w, h = bbox[i]
            a = w * h
            c = [(xc - w / two) * fw, (yc - h / two) * fh, (xc + w / two) * fw, (yc + h / two) * fh]
            assert all(isinstance(v, np.float32) for v in c + [a])
            if np.isnan(a) or any(np.isnan(v) for v in c):
                continue
            todo.append((a, i, [_trunc_i32(v) for v in c]))
    todo.sort(key=lambda t: t[0], reverse=True)          # stable: ties keep slot order
    for _, i, (X1, Y1, X2, Y2) in todo:
        if X1 > X2:
            X1, X2 = X2, X1
        if Y1 > Y2:
            Y1, Y2 = Y2, Y1
        col = np.asarray(colors[int(labels[i])], np.int64)
        xa, xb, ya, yb = max(X1, 0), min(X2, W - 1), max(Y1, 0), min(Y2, H - 1)
        if xa > xb or ya > yb:
            continue
        d = img[ya:yb + 1, xa:xb + 1].astype(np.int64)
        t = col.reshape(1, 1, 3) * 100 + d * 155 + 128
        d = ((t >> 8) + t) >> 8
        ys = np.arange(ya, yb + 1).reshape(-1, 1)
        xs = np.arange(xa, xb + 1).reshape(1, -1)
        border = (ys == Y1) | (ys == Y2) | (xs == X1) | (xs == X2)
        d[border] = col
        img[ya:yb + 1, xa:xb + 1] = d.astype(np.uint8)
    return img


def cell_size(W, H, S):
    """Rule 4."""
    if W > H:
        return S, int(float(H) / float(W) * float(S)) // 2 * 2
    return int(float(W) / float(H) * float(S)) // 2 * 2, S


def cell(bbox, valid, labels, colors, W, H, S, page=None):
    """Rules 1-6 -> uint8 [S, S, 3]."""
    assert S % 2 == 0
    Wn, Hn = cell_size(W, H, S)
    assert Wn >= 1 and Hn >= 1
    small = resize_bilinear_u8(draw(bbox, valid, labels, colors, W, H, page), Hn, Wn)
    out = np.zeros((S, S, 3), np.uint8)
    if W > H:
        out[(S - Hn) // 2:(S - Hn) // 2 + Hn, :Wn] = small
    elif H > W:
        out[:Hn, (S - Wn) // 2:(S - Wn) // 2 + Wn] = small
    else:
        out[:] = small
    return out


def make_grid(cells, nrow=None):
    """Rule 7: torchvision's make_grid(padding=2, pad_value=0) of uint8 [B, S, S, 3] cells -> [Hg, Wg, 3]."""
    cells = np.asarray(cells)
    B, S = cells.shape[0], cells.shape[1]
    if B == 1:
        return cells[0].copy()
    if nrow is None:
        nrow = int(np.ceil(np.sqrt(B)))
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(float(B) / xmaps))
    out = np.zeros((ymaps * (S + 2) + 2, xmaps * (S + 2) + 2, 3), np.uint8)
    for k in range(B):
        r, c = 2 + (k // xmaps) * (S + 2), 2 + (k % xmaps) * (S + 2)
        out[r:r + S, c:c + S] = cells[k]
    return out


def grid(bbox, valid, labels, colors, page_wh, S, pages=None, page_index=None, nrow=None):
    """Rules 1-7 for a batch: bbox [B, N, 4], valid / labels [B, N], page_wh (W, H) or [B, 2], pages = list of uint8 [H, W, 3] or None."""
    B = len(bbox)
    wh = np.broadcast_to(np.asarray(page_wh).reshape(-1, 2), (B, 2))
    cells = []
    for b in range(B):
        pg = None
        if pages is not None:
            k = b if page_index is None else int(page_index[b])
            pg = pages[k] if k >= 0 else None
        cells.append(cell(bbox[b], valid[b], labels[b], colors, int(wh[b, 0]), int(wh[b, 1]), S, pg))
    return make_grid(np.stack(cells), nrow)
