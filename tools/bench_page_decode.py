"""Loader cost of the page backgrounds under LayoutDataset mode='device' (Pillow inflates + unfilters the page on the host) and mode='raw' (the PNG
bytes go to the GPU, csrc/png_decode.hip decodes them): a zip written the way the reference's dataset_tool.py:325-363 writes it (ZIP_STORED entries,
PNGs saved with compress_level=0, optimize=False) with 16 pages of 1024 x 1024 (half smooth, half noise), and a second one with one 4096 x 4096 page.
Per dataset:
  (a) host ms per item of mode='device' __getitem__                      (the yardstick: what every item costs today)
  (b) host ms per item of mode='raw' __getitem__ (read + scan), without and with verify_png=True
  (c) the decode call alone for the batch, us, gather and unfilter apart, next to the resize of the same pages (csrc/resample.hip)
  (d) pages/s of the in-process route (__getitem__ x n, collate, batch_backgrounds_to_device, synchronise) under both modes, alternating
Medians after a warm-up.  Prints the figures and one JSON line (kept in profiles/page_decode_bench.json).
usage: python tools/bench_page_decode.py [--json PATH]"""
import io
import json
import os
import sys
import tempfile
import time
import zipfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from layoutdetr_amd.training import dataset_layoutganpp as D

STEP_MS = (32.1, 32.6)          # README.md: the training step at batch 16 on one MI355X
PASSES = 5


def page(side, kind, seed):
    rs = np.random.RandomState(seed)
    if kind == 'noise':
        return rs.randint(0, 256, size=(side, side, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:side, 0:side]
    base = np.stack([(xx * 255) // side, (yy * 255) // side, ((xx + yy) * 127) // side], -1)
    return np.clip(base + rs.randint(-3, 4, size=base.shape), 0, 255).astype(np.uint8)      # a gradient with sensor-like noise


def png_bytes(arr):
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(arr).save(buf, format='png', compress_level=0, optimize=False)
    return buf.getvalue()


def write_zip(path, pages):
    samples = []
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_STORED) as z:
        for i, p in enumerate(pages):
            base = f'page{i:03d}'
            samples.append([base, dict(bboxes=[[0.5, 0.5, 0.4, 0.2]], labels=[1], texts=['bench'], page_label=0,
                                       attr=dict(name=base, width=p.shape[1], height=p.shape[0], num_bbox_labels=8))])
            z.writestr(base + '_background_orig.png', png_bytes(p))
            z.writestr(base + '_0_patch_orig.png', png_bytes(np.zeros((8, 8, 3), np.uint8)))
        z.writestr('non_image.json', json.dumps(dict(samples=samples)))


def median(xs):
    return sorted(xs)[len(xs) // 2]


def item_ms(ds):
    """Median over PASSES of the mean host milliseconds of one __getitem__."""
    n = len(ds)
    for i in range(n):
        ds[i]
    out = []
    for _ in range(PASSES):
        t = time.perf_counter()
        for i in range(n):
            ds[i]
        out.append((time.perf_counter() - t) * 1e3 / n)
    return median(out)


def event_us(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(PASSES):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / reps * 1e3)
    return median(times)


def route_pages_per_s(datasets, size, dev):
    """{mode: pages/s} of __getitem__ x n + collate + batch_backgrounds_to_device + synchronise, the modes alternating pass by pass."""
    times = {m: [] for m in datasets}
    for rep in range(PASSES + 1):
        for m, ds in datasets.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            samples, _ = ds.collate([ds[i] for i in range(len(ds))])
            out = D.batch_backgrounds_to_device(samples['background'], size, dev)
            torch.cuda.synchronize()
            if rep:                                                  # pass 0 warms up
                times[m].append(time.perf_counter() - t)
            del out
    return {m: len(datasets[m]) / median(v) for m, v in times.items()}


def bench(path, size, dev):
    ds = {m: D.LayoutDataset(path=path, background_size=size, mode=m) for m in ('device', 'raw')}
    n = len(ds['raw'])
    row = dict(pages=n, side=int(ds['raw'][0][0]['background'].height), file_bytes=int(ds['raw'][0][0]['background'].data.size))
    row['a_device_getitem_ms'] = item_ms(ds['device'])
    row['b_raw_getitem_ms'] = item_ms(ds['raw'])
    row['b_raw_getitem_verify_ms'] = item_ms(D.LayoutDataset(path=path, background_size=size, mode='raw', verify_png=True))
    raws = [ds['raw'][i][0]['background'] for i in range(n)]
    assert all(isinstance(r, D.RawPage) for r in raws), 'a page of the bench set fell back to Pillow'
    row['segments_per_page'] = float(np.mean([len(r.segments) for r in raws]))
    row['row_ranges_per_page'] = float(np.mean([len(r.row_starts) for r in raws]))
    state = {}
    pages = D._decode_group(raws, dev, state=state)                  # uploads once; the timed calls below reuse the buffers
    want = torch.from_numpy(np.stack([ds['device'][i][0]['background'] for i in range(n)]))
    assert torch.equal(pages.cpu(), want), 'the device decode differs from Pillow'
    row['c_gather_us'] = event_us(lambda: D._decode_group(raws, dev, phases=1, state=state))
    row['c_unfilter_us'] = event_us(lambda: D._decode_group(raws, dev, phases=2, state=state))
    row['c_decode_us'] = event_us(lambda: D._decode_group(raws, dev, phases=3, state=state))
    row['c_resize_us'] = event_us(lambda: D.background_to_tensor(pages, size))
    row['c_decode_share_of_step'] = [row['c_decode_us'] / 1e3 / s for s in STEP_MS]
    pps = route_pages_per_s(ds, size, dev)
    row['d_device_pages_per_s'], row['d_raw_pages_per_s'] = pps['device'], pps['raw']
    row['host_cores_freed_per_gpu'] = [16 * (row['a_device_getitem_ms'] - row['b_raw_getitem_ms']) / s for s in STEP_MS]
    print(f"{n} x {row['side']}^2: (a) device __getitem__ {row['a_device_getitem_ms']:.2f} ms/item; (b) raw {row['b_raw_getitem_ms']:.3f} ms/item, "
          f"verify {row['b_raw_getitem_verify_ms']:.2f}; (c) decode {row['c_decode_us']:.0f} us = gather {row['c_gather_us']:.0f} + unfilter {row['c_unfilter_us']:.0f} "
          f"(resize {row['c_resize_us']:.0f} us), {100 * row['c_decode_share_of_step'][0]:.2f} % of the step; (d) {pps['device']:.0f} pages/s device, {pps['raw']:.0f} raw; "
          f"host cores freed per GPU {row['host_cores_freed_per_gpu'][1]:.2f}-{row['host_cores_freed_per_gpu'][0]:.2f}")
    return row


def main():
    out_path = sys.argv[sys.argv.index('--json') + 1] if '--json' in sys.argv else None
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        small, big = os.path.join(tmp, 'pages1024.zip'), os.path.join(tmp, 'page4096.zip')
        write_zip(small, [page(1024, 'smooth' if i % 2 == 0 else 'noise', i) for i in range(16)])
        write_zip(big, [page(4096, 'smooth', 99)])
        rows.append(bench(small, 1024, dev))
        rows.append(bench(big, 1024, dev))
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), host_cpus=len(os.sched_getaffinity(0)), passes=PASSES, step_ms=STEP_MS, rows=rows))
    print(line)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
