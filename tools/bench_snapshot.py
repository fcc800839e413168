"""Measurements behind the image snapshots (layoutdetr_amd/render.py, csrc/layout_raster.hip) -> profiles/snapshot_bench.json, one JSON line on stdout.

    python tools/bench_snapshot.py [--out profiles/snapshot_bench.json]

Configurations: B = 64 layouts of 9 boxes on white 1200 x 628 pages, canvas 128 (a `*_layouts_*` grid); B = 16 over 1200 x 628 uint8 pages, canvas 256 (a
`*_layouts_over_background_*` grid).
  (a) reference_procedure   the reference's save_image (util.py:85-141) RESTATED here: per sample `boxes[i][mask]` on device tensors, fp32 0-d tensor arithmetic,
                            one ImageDraw.rectangle per element on a page-sized canvas, a PIL BILINEAR resize, expand2square, the grid assembled with numpy in
                            place of ToTensor / make_grid (torchvision is not installed), PIL's PNG encoder
  (b) grid_and_png          render.layout_grid + render.save_png: one launch, one device-to-host copy, PIL's PNG encoder
  (c) launch                render.layout_grid alone
Method (as tools/bench_generate.py): warm-up, then blocks of calls that last at least 0.2 s (at least 3 calls), each block timed by a pair of device events
(`*_us`) and by a host clock between two synchronisations (`host_*_us`); the versions alternate, 5 blocks each; median, minimum and maximum per call.  Kernel
launches per call are counted by torch.profiler.  (a) is bound by the host; what a training tick waits for is the host figure."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_generate import alternate, launches  # noqa: E402


def reference_cell(boxes, labels, colors, W_page, H_page, size_canvas, page=None):
    """util.py:85-112 restated (the canvas starts as `page` for the over-background kind)."""
    from PIL import Image, ImageDraw
    img = Image.new('RGB', (W_page, H_page), color=(255, 255, 255)) if page is None else Image.fromarray(page, 'RGB')
    draw = ImageDraw.Draw(img, 'RGBA')
    area = [b[2] * b[3] for b in boxes]
    for i in sorted(range(len(area)), key=lambda i: area[i], reverse=True):
        bbox, color = boxes[i], colors[labels[i]]
        xc, yc, w, h = bbox
        x1, y1, x2, y2 = xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2
        draw.rectangle([float(x1 * W_page), float(y1 * H_page), float(x2 * W_page), float(y2 * H_page)], outline=color, fill=color + (100,))
    if W_page > H_page:
        wn, hn = size_canvas, int(float(H_page) / float(W_page) * float(size_canvas)) // 2 * 2
    else:
        wn, hn = int(float(W_page) / float(H_page) * float(size_canvas)) // 2 * 2, size_canvas
    img = img.resize((wn, hn), resample=Image.BILINEAR)
    out = Image.new('RGB', (size_canvas, size_canvas), color=(0, 0, 0))
    out.paste(img, (0, (size_canvas - hn) // 2) if W_page > H_page else ((size_canvas - wn) // 2, 0))
    return out


def reference_save_image(bbox, labels, mask, colors, path, W, H, S, pages=None):
    """util.py:115-141 restated: the per-sample loop over DEVICE tensors, then the grid (numpy in place of make_grid) and the PNG."""
    from PIL import Image
    B = bbox.size(0)
    cells = []
    for i in range(B):
        m = mask[i]
        cells.append(np.array(reference_cell(bbox[i][m], labels[i][m], colors, W, H, S, None if pages is None else pages[i])))
    nrow = int(np.ceil(np.sqrt(B)))
    ymaps = int(np.ceil(B / nrow))
    grid = np.zeros((ymaps * (S + 2) + 2, nrow * (S + 2) + 2, 3), np.uint8)
    for k, c in enumerate(cells):
        grid[2 + (k // nrow) * (S + 2):2 + (k // nrow) * (S + 2) + S, 2 + (k % nrow) * (S + 2):2 + (k % nrow) * (S + 2) + S] = c
    Image.fromarray(grid, 'RGB').save(path)
    return grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'snapshot_bench.json'))
    args = ap.parse_args()
    from layoutdetr_amd import render
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    colors = [(246, 85, 85), (246, 205, 85), (165, 246, 85), (85, 246, 125), (85, 246, 246), (85, 125, 246), (165, 85, 246), (246, 85, 205)]
    W, H = 1200, 628
    res = dict(device=torch.cuda.get_device_name(0), page=[W, H], boxes_per_layout=9,
               method='device events (and, host_*, a synchronised host clock) around >= 0.2 s blocks of calls (>= 3); versions alternated; 5 blocks; median [min, max] in us per call',
               cases={})
    tmp = tempfile.mkdtemp()
    for name, B, S, over in (('layouts_B64_canvas128', 64, 128, False), ('over_background_B16_canvas256', 16, 256, True)):
        bbox = torch.cat([torch.rand(B, 9, 2, generator=g) * 0.6 + 0.2, torch.rand(B, 9, 2, generator=g) * 0.4 + 0.05], -1).to(dev)
        mask = (torch.arange(9)[None, :] < torch.randint(3, 10, (B, 1), generator=g))
        labels = torch.randint(0, 8, (B, 9), generator=g)
        pages_h = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g) if over else None
        pages = render.PageSet(list(pages_h.to(dev))) if over else None
        pages_np = pages_h.numpy() if over else None
        mask_d, labels_d = mask.to(dev), labels.to(dev)

        def reference_procedure():
            return reference_save_image(bbox, labels_d, mask_d, colors, os.path.join(tmp, 'a.png'), W, H, S, pages_np)

        def launch():
            return render.layout_grid(bbox, mask, labels, colors, (W, H), pages=pages, canvas=S)

        def grid_and_png():
            render.save_png(launch(), os.path.join(tmp, 'b.png'))
        same = bool(np.array_equal(reference_procedure(), launch().cpu().numpy()))
        r = alternate(dict(reference_procedure=reference_procedure, grid_and_png=grid_and_png, launch=launch), warmup=1)
        for k, fn in (('reference_procedure', reference_procedure), ('grid_and_png', grid_and_png), ('launch', launch)):
            r[k]['launches'] = launches(fn)
        r['pixels_equal_reference_procedure'] = same
        r['one_snapshot_adds_ms_host'] = r['grid_and_png']['host_median_us'] * 1e-3
        res['cases'][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
