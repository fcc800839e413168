"""Measurements behind the device PNG encoder (layoutdetr_amd/render.py encode_png, csrc/png_encode.hip) -> profiles/png_encode_bench.json, one JSON line
on stdout.

    python tools/bench_png_encode.py [--out profiles/png_encode_bench.json]

The four snapshot grids of tools/bench_snapshot.py, each built ONCE on the device: `layouts` B = 64 at canvas 128, `layouts_over_background`
B = 16 at canvas 256 over noise pages, `images` and `images_with_background` B = 16 at canvas 1024 (4106 x 4106).  Per grid, in ONE run:
  (a) save_pillow     render.save_png(grid, path, encoder='pillow'): the pixels copied to the host, Pillow's encoder, the file written
  (b) save_device     render.save_png(grid, path, encoder='device'): three launches, the length and the file's bytes copied, the file written
  (c) encode_launches the three launches of ldetr_png_encode_u8 alone on preallocated buffers: no copy, no file
Method (tools/bench_generate.py): warm-up, then blocks of calls that last at least 0.2 s (at least 2 calls), each block timed by a pair of device events
(`*_us`) and by a host clock between two synchronisations (`host_*_us`); the versions alternate, 5 blocks each; median, minimum and maximum per call.
What a training tick waits for is the host figure.  Accepted when, in every case, the maximum of (b) is below the minimum of (a)."""
import argparse
import ctypes
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


def grids(render, dev):
    """name -> uint8 [H, W, 3] device grid, the four configurations of tools/bench_snapshot.py."""
    g = torch.Generator().manual_seed(0)
    colors = [(246, 85, 85), (246, 205, 85), (165, 246, 85), (85, 246, 125), (85, 246, 246), (85, 125, 246), (165, 85, 246), (246, 85, 205)]
    W, H = 1200, 628
    out = {}
    for name, B, S, over in (('layouts_B64_canvas128', 64, 128, False), ('over_background_B16_canvas256', 16, 256, True)):
        bbox = torch.cat([torch.rand(B, 9, 2, generator=g) * 0.6 + 0.2, torch.rand(B, 9, 2, generator=g) * 0.4 + 0.05], -1).to(dev)
        mask = (torch.arange(9)[None, :] < torch.randint(3, 10, (B, 1), generator=g))
        labels = torch.randint(0, 8, (B, 9), generator=g)
        pages = render.PageSet(list(torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev))) if over else None
        out[name] = render.layout_grid(bbox, mask, labels, colors, (W, H), pages=pages, canvas=S)
    B, N, S = 16, 9, 1024
    coarse = torch.rand(B * N, 3, H // 8 + 1, W // 8 + 1, generator=g).to(dev)            # smooth page-sized canvases: text patches are not noise
    canv = (torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False) * 255.0).round().clamp(0, 255).to(torch.uint8).view(B, N, 3, H, W)
    real = torch.cat([torch.rand(B, N, 2, generator=g) * 0.6 + 0.2, torch.rand(B, N, 2, generator=g) * 0.4 + 0.05], -1)
    fake = torch.cat([torch.rand(B, N, 2, generator=g) * 0.6 + 0.2, torch.rand(B, N, 2, generator=g) * 0.4 + 0.05], -1).to(dev)
    mask = torch.ones(B, N, dtype=torch.bool)
    crops = []
    for b in range(B):
        row = []
        for i in range(N):
            w, h = int(real[b, i, 2] * W), int(real[b, i, 3] * H)
            row.append(canv[b, i, :, H // 2 - h // 2:H // 2 + h - h // 2, W // 2 - w // 2:W // 2 + w - w // 2].permute(1, 2, 0).contiguous())
        crops.append(row)
    patches = render.PatchSet(crops, dev)
    bg = torch.rand(B, 3, 129, 129, generator=g).to(dev)
    bg = (torch.nn.functional.interpolate(bg, size=(1024, 1024), mode='bilinear', align_corners=False) * 255.0).round().clamp(0, 255).to(torch.uint8)
    pages = render.PageSet(list(bg.permute(0, 2, 3, 1).contiguous()))
    out['images_B16_canvas1024'] = render.image_grid(fake, real, mask, patches, (W, H), canvas=S)
    out['images_with_background_B16_canvas1024'] = render.image_grid(fake, real, mask, patches, (W, H), backgrounds=pages, canvas=S)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_encode_bench.json'))
    args = ap.parse_args()
    import PIL.Image
    from layoutdetr_amd import _lib, render
    from layoutdetr_amd.hip import core
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), segment_bytes=render.PNG_ENCODE_SEGMENT,
               method='device events (and, host_*, a synchronised host clock) around >= 0.2 s blocks of calls (>= 2); versions alternated; 5 blocks; median [min, max] in us per call',
               cases={})
    tmp = tempfile.mkdtemp()
    ok = True
    for name, grid in grids(render, dev).items():
        Hg, Wg = int(grid.shape[0]), int(grid.shape[1])
        pa, pb = os.path.join(tmp, 'a.png'), os.path.join(tmp, 'b.png')
        bound, ws_bytes = render.png_encode_bound(Hg, Wg)
        out = torch.empty(bound, dtype=torch.uint8, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        a = _lib.PngEncodeArgs(struct_bytes=ctypes.sizeof(_lib.PngEncodeArgs), H=Hg, W=Wg, blocks=0, filter=-1, reserved=0, src=grid.data_ptr(), out=out.data_ptr(),
                               out_capacity=bound, total_bytes=total.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws_bytes, seg_table=None, seg_table_rows=0)

        def save_pillow():
            render.save_png(grid, pa, encoder='pillow')

        def save_device():
            render.save_png(grid, pb, encoder='device')

        def encode_launches():
            core.check(core.lib().ldetr_png_encode_u8(ctypes.byref(a), core.stream()), 'png_encode_u8')
        r = alternate(dict(save_pillow=save_pillow, save_device=save_device, encode_launches=encode_launches), warmup=1, min_calls=2)
        same = bool(np.array_equal(np.array(PIL.Image.open(pb)), grid.cpu().numpy()))
        data, stats = render.encode_png(grid, return_stats=True)
        types = np.bincount(stats['segments'][:, 2], minlength=3)
        r['encode_launches']['launches'] = launches(encode_launches)
        r.update(grid=[Wg, Hg], raw_bytes=Hg * (1 + 3 * Wg), pillow_file_bytes=os.path.getsize(pa), device_file_bytes=os.path.getsize(pb),
                 size_ratio_to_pillow=os.path.getsize(pb) / os.path.getsize(pa), bytes_to_host_pillow=grid.numel(), bytes_to_host_device=int(data.numel()) + 8,
                 segments=dict(stored=int(types[0]), fixed=int(types[1]), dynamic=int(types[2])), device_file_decodes_to_the_grid=same,
                 device_max_below_pillow_min=bool(r['save_device']['host_max_us'] < r['save_pillow']['host_min_us']),
                 speedup_host_median=r['save_pillow']['host_median_us'] / r['save_device']['host_median_us'])
        ok = ok and same and r['device_max_below_pillow_min']
        res['cases'][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        del out, ws
    res['accepted'] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
