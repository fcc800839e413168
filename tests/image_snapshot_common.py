"""Numpy restatements of the `images` snapshot kinds (DESIGN.md §13 rules 8-12; the reference's util.py:144-325), shared by
test_image_snapshot_cpu.py, test_image_snapshot_gpu.py, tools/gen_image_snapshot_golden.py and tools/bench_snapshot.py.  Independent of the package:
nothing here imports layoutdetr_amd.

Two restatements of the same procedure:
* `*_f32`: the package's rule, in fp32, sequential in the stated order -- what the kernels must give bit for bit.
* `*_f64`: what the reference computes -- float64 throughout, skimage.transform.resize(anti_aliasing=True) in the closed form on which
  scipy.ndimage's gaussian_filter(mode='mirror') and zoom(order=1, mode='mirror', grid_mode=True) agree to 3e-16, `(img * 255).astype('ubyte')` at the end.
The tail (PIL BILINEAR resize, letterbox, make_grid: rules 4-7) is snapshot_common's."""
import numpy as np

import snapshot_common as SC

RGB_MEAN = np.array([0.485, 0.456, 0.406], np.float32).reshape(1, 1, 3)
RGB_STD = np.array([0.229, 0.224, 0.225], np.float32).reshape(1, 1, 3)
BIAS = np.float32(2.0 ** -10)


def mirror(i, n):
    """scipy.ndimage's `mirror` boundary: period 2 (n - 1), reflected; n == 1 -> 0."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m >= n, p - m, m)


def axis_table(n_in, n_out):
    """Rule 10 for one axis, in double: (radius, Gaussian weights [2r + 1], i0, i1 (mirror-mapped), w0 = 1 - t, w1 = t)."""
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
    return r, g, mirror(i0, n_in), mirror(i0 + 1, n_in), 1.0 - t, t


def _resize(v, ho, wo, dtype):
    """Gaussian along axis 0, then 1 (each sum starts at 0 and adds weight * value for k = -r .. r); then interpolation along axis 0, then 1, as
    (w0 * a) + (w1 * b).  Every operation is one rounding in `dtype`."""
    tabs = [axis_table(v.shape[0], ho), axis_table(v.shape[1], wo)]
    for axis, (r, g, _, _, _, _) in enumerate(tabs):
        if r == 0:
            continue
        n = v.shape[axis]
        g = g.astype(dtype)
        acc = np.zeros_like(v)
        for k in range(-r, r + 1):
            acc = acc + g[k + r] * np.take(v, mirror(np.arange(n) + k, n), axis=axis)
        v = acc
    for axis, (_, _, i0, i1, w0, w1) in enumerate(tabs):
        shape = [1, 1, 1]
        shape[axis] = -1
        w0, w1 = w0.astype(dtype).reshape(shape), w1.astype(dtype).reshape(shape)
        v = (w0 * np.take(v, i0, axis=axis)) + (w1 * np.take(v, i1, axis=axis))
    assert v.dtype == dtype
    return v


def resize_f32(img, ho, wo):
    """Rule 10 on a uint8 [h, w, 3] image -> uint8 [ho, wo, 3], fp32: u8 / 255, the passes, clamp to [0, 1], floor(v * 255 + 2^-10)."""
    v = np.asarray(img, np.uint8).astype(np.float32) / np.float32(255)
    v = np.clip(_resize(v, ho, wo, np.float32), np.float32(0), np.float32(1))
    q = np.floor(v * np.float32(255) + BIAS)
    assert q.dtype == np.float32
    return q.astype(np.uint8)


def resize_f64(im, ho, wo):
    """skimage.transform.resize(im, (ho, wo), anti_aliasing=True) of a float [h, w, 3] image in float64, clipped to the input's range."""
    im = np.asarray(im, np.float64)
    return np.clip(_resize(im, ho, wo, np.float64), im.min(), im.max())


def crop_window(canvas_hw, bbox_real, W, H):
    """Rule 8: (y0, y1, x0, x1) of the centre window of a [Hc, Wc] canvas, or None when it is empty or leaves the canvas."""
    b = np.asarray(bbox_real, np.float32)
    width, height = int(b[2] * np.float32(W)), int(b[3] * np.float32(H))
    cy, cx = canvas_hw[0] // 2, canvas_hw[1] // 2
    y0, y1, x0, x1 = cy - height // 2, cy + height - height // 2, cx - width // 2, cx + width - width // 2
    if width < 1 or height < 1 or y0 < 0 or x0 < 0 or y1 > canvas_hw[0] or x1 > canvas_hw[1]:
        return None
    return y0, y1, x0, x1


def paste_rect(bbox_fake, W, H):
    """Rule 9: the fp32 corners (xc -+ w / 2) * W, (yc -+ h / 2) * H rounded half to even -> (x1, y1, x2, y2), or None for a NaN corner."""
    xc, yc, w, h = np.asarray(bbox_fake, np.float32)
    two, fw, fh = np.float32(2), np.float32(W), np.float32(H)
    with np.errstate(all='ignore'):
        c = [(xc - w / two) * fw, (yc - h / two) * fh, (xc + w / two) * fw, (yc + h / two) * fh]
    assert all(isinstance(v, np.float32) for v in c)
    if any(np.isnan(v) for v in c):
        return None
    return tuple(int(np.clip(np.rint(np.float64(v)), -2 ** 30, 2 ** 30)) for v in c)


def draw_order(bbox_fake, valid):
    """Stable descending fp32 w * h of the fake boxes over the valid slots; a NaN area is skipped."""
    b = np.asarray(bbox_fake, np.float32)
    with np.errstate(all='ignore'):
        todo = [(b[i, 2] * b[i, 3], i) for i in range(b.shape[0]) if valid[i]]
    todo = [t for t in todo if not np.isnan(t[0])]
    todo.sort(key=lambda t: t[0], reverse=True)
    return [i for _, i in todo]


def jobs_of_cell(bbox_fake, valid, crops, W, H):
    """[(slot, crop, (x1, y1, x2, y2))] in draw order: the elements that draw something (rules 8, 9)."""
    out = []
    for i in draw_order(bbox_fake, valid):
        r = paste_rect(bbox_fake[i], W, H)
        if crops[i] is None or r is None:
            continue
        x1, y1, x2, y2 = r
        if x2 <= x1 or y2 <= y1 or x2 <= 0 or y2 <= 0 or x1 >= W or y1 >= H:
            continue
        out.append((i, crops[i], r))
    return out


def page_f32(bbox_fake, valid, crops, W, H, background=None):
    """Rules 8-11 -> the uint8 [H, W, 3] page."""
    img = np.full((H, W, 3), 255, np.uint8) if background is None else resize_f32(background, H, W)
    for _, crop, (x1, y1, x2, y2) in jobs_of_cell(bbox_fake, valid, crops, W, H):
        im = resize_f32(crop, y2 - y1, x2 - x1)
        xa, xb, ya, yb = max(x1, 0), min(x2, W), max(y1, 0), min(y2, H)
        img[ya:yb, xa:xb] = im[ya - y1:yb - y1, xa - x1:xb - x1]
    return img


def page_f64(bbox_fake, valid, crops, W, H, background=None):
    """The reference's procedure (util.py:144-194 / :234-285) in float64 on exact u8 / 255 inputs -> uint8 [H, W, 3]."""
    img = np.ones((H, W, 3), np.float64) if background is None else resize_f64(np.asarray(background, np.float64) / 255.0, H, W)
    for _, crop, (x1, y1, x2, y2) in jobs_of_cell(bbox_fake, valid, crops, W, H):
        im = resize_f64(np.asarray(crop, np.float64) / 255.0, y2 - y1, x2 - x1)
        xa, xb, ya, yb = max(x1, 0), min(x2, W), max(y1, 0), min(y2, H)
        img[ya:yb, xa:xb] = im[ya - y1:yb - y1, xa - x1:xb - x1]
    return (img * 255.0).astype(np.uint8)


def letterbox(page, S):
    """Rules 4-6 (rule 12 here): PIL BILINEAR resize to the cell size, expand2square."""
    H, W = page.shape[:2]
    Wn, Hn = SC.cell_size(W, H, S)
    assert Wn >= 1 and Hn >= 1
    small = SC.resize_bilinear_u8(page, Hn, Wn)
    out = np.zeros((S, S, 3), np.uint8)
    if W > H:
        out[(S - Hn) // 2:(S - Hn) // 2 + Hn, :Wn] = small
    elif H > W:
        out[:Hn, (S - Wn) // 2:(S - Wn) // 2 + Wn] = small
    else:
        out[:] = small
    return out


def cell_f32(bbox_fake, valid, crops, W, H, S, background=None):
    return letterbox(page_f32(bbox_fake, valid, crops, W, H, background), S)


def cell_f64(bbox_fake, valid, crops, W, H, S, background=None):
    return letterbox(page_f64(bbox_fake, valid, crops, W, H, background), S)


def grid_f32(bbox_fake, valid, crops, page_wh, S, backgrounds=None, nrow=None):
    """Rules 8-12 and make_grid for a batch: crops[b] = list of N entries; backgrounds = list of uint8 images or None."""
    B = len(bbox_fake)
    wh = np.broadcast_to(np.asarray(page_wh).reshape(-1, 2), (B, 2))
    cells = [cell_f32(bbox_fake[b], valid[b], crops[b], int(wh[b, 0]), int(wh[b, 1]), S, None if backgrounds is None else backgrounds[b]) for b in range(B)]
    return SC.make_grid(np.stack(cells), nrow)


def keeps_a_size(bbox_fake, valid, crops, W, H, background=None):
    """Whether any resize job of the cell keeps its size on an axis (identity-size jobs are judged separately: DESIGN.md §13)."""
    jobs = [(c.shape[:2], (y2 - y1, x2 - x1)) for _, c, (x1, y1, x2, y2) in jobs_of_cell(bbox_fake, valid, crops, W, H)]
    if background is not None:
        jobs.append((background.shape[:2], (H, W)))
    return any(a[0] == b[0] or a[1] == b[1] for a, b in jobs)


def unpack_crops(buf, table):
    """Fixture storage -> crops[b][i]: `table` [B, N, 3] = (offset, w, h), offset -1 = no crop; `buf` the concatenated uint8 bytes."""
    out = []
    for b in range(table.shape[0]):
        row = []
        for off, w, h in table[b]:
            row.append(None if off < 0 else np.asarray(buf[off:off + h * w * 3]).reshape(h, w, 3))
        out.append(row)
    return out


def pack_crops(crops):
    n = max(len(c) for c in crops)
    table = np.full((len(crops), n, 3), -1, np.int64)
    parts, at = [], 0
    for b, row in enumerate(crops):
        for i, c in enumerate(row):
            if c is None:
                continue
            table[b, i] = (at, c.shape[1], c.shape[0])
            parts.append(np.ascontiguousarray(c).reshape(-1))
            at += c.size
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), table
