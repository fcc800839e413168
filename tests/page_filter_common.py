"""Numpy restatement of the two 8-bit page filters of csrc/page_filter.hip, the yardstick of tests/test_page_filter_*.py.

Blur = Pillow's GaussianBlur (src/libImaging/BoxBlur.c): the Gaussian radius becomes one fractional box radius, the box runs three times along
x and then three times along y, and every pass is rounded to 8 bits.  Edge = convert('L').filter(FIND_EDGES).convert('RGB').  Integer
arithmetic throughout, so "equal" means bit for bit."""
import numpy as np

SIZES = [(1, 1), (1, 7), (2, 9), (3, 2), (3, 3), (5, 3), (7, 6), (33, 17), (64, 131)]      # (H, W)


def box_radius(radius, passes=3):
    """Gaussian radius -> (r, ww, fw): integer box radius and the 24-bit fixed-point weights of an inner and of an edge pixel.
    Pillow's `_gaussian_blur_radius` keeps sigma2, L, l and a in C `float`s: the square root and the floor are taken in double and rounded
    to float on assignment, the products and the quotient of `a` are float operations.  (Evaluated in double instead, ww comes out one
    unit different at a few radii, 0.3 and 1.35 among them, and pixels differ from Pillow's.)"""
    f = np.float32
    s2 = f(f(radius) * f(radius)) / f(passes)
    L = f(np.sqrt(12.0 * float(s2) + 1.0))
    l = f(np.floor((float(L) - 1.0) / 2.0))
    a = f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * s2))
    a = f(a / f(f(6) * f(s2 - f(f(l + f(1)) * f(l + f(1))))))
    fr = f(l + a)
    r = int(fr)
    ww = int(f(1 << 24) / (fr * f(2) + f(1)))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def box_pass(a, r, ww, fw):
    """One pass along the LAST axis of a uint8 array, indices clamped to the line."""
    n = a.shape[-1]
    src = a.astype(np.uint64)
    x = np.arange(n)
    acc = np.zeros(a.shape, np.uint64)
    for d in range(-r, r + 1):
        acc += src[..., np.clip(x + d, 0, n - 1)]
    edge = src[..., np.clip(x - r - 1, 0, n - 1)] + src[..., np.clip(x + r + 1, 0, n - 1)]
    out = (np.uint64(ww) * acc + np.uint64(fw) * edge + np.uint64(1 << 23)) >> np.uint64(24)
    assert int(out.max(initial=0)) <= 255
    return out.astype(np.uint8)


def blur(page, radius=3.0):
    """page: uint8 [..., H, W, 3] -> GaussianBlur(radius)."""
    r, ww, fw = box_radius(radius)
    a = np.moveaxis(np.asarray(page), -2, -1)              # [..., H, 3, W]: x last
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    a = np.moveaxis(a, -3, -1)                             # [..., 3, W, H]: y last
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    return np.ascontiguousarray(np.moveaxis(a, (-3, -2, -1), (-1, -2, -3)))


def grey(page):
    p = np.asarray(page).astype(np.uint32)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16).astype(np.uint8)


def edge(page):
    """page: uint8 [..., H, W, 3] -> convert('L').filter(FIND_EDGES).convert('RGB')."""
    g = grey(page)
    H, W = g.shape[-2:]
    out = g.copy()
    if H >= 3 and W >= 3:
        gi = g.astype(np.int32)
        s = np.zeros(gi[..., 1:-1, 1:-1].shape, np.int32)
        for dy in range(3):
            for dx in range(3):
                s += gi[..., dy:H - 2 + dy, dx:W - 2 + dx]
        out[..., 1:-1, 1:-1] = np.clip(9 * gi[..., 1:-1, 1:-1] - s, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(out[..., None], 3, axis=-1))


FILTERS = {'blur': blur, 'edge': edge}


def pillow_filter(page, kind, radius=3.0):
    """The same filters by Pillow itself (generate.py:267-269, 280-282 of the reference)."""
    from PIL import Image, ImageFilter
    img = Image.fromarray(np.ascontiguousarray(page))
    if kind == 'blur':
        return np.array(img.filter(ImageFilter.GaussianBlur(radius=radius)))
    if kind == 'edge':
        return np.array(img.convert('L').filter(ImageFilter.FIND_EDGES).convert('RGB'))
    raise ValueError(kind)


def pages(rng, shape, pattern):
    """Test pages: 'random' bytes, or a 0/255 'checker' board with squares of 1..3 pixels per channel (rounding at saturation)."""
    H, W = shape[-3:-1]
    if pattern == 'random':
        return rng.randint(0, 256, size=shape).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    planes = [(((y // (c + 1)) + (x // (c + 1))) % 2 * 255).astype(np.uint8) for c in range(3)]
    return np.broadcast_to(np.stack(planes, -1), shape).copy()
