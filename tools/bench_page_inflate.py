"""Loader cost of the page backgrounds under LayoutDataset mode='packed' (indexed compressed PNGs inflated on the GPU, csrc/png_inflate.hip) next to
mode='device' on the SAME compressed files (Pillow inflates on the host) and mode='raw' on stored-block files of the same pages (csrc/png_decode.hip).
Method of tools/bench_page_decode.py (medians of 5 passes after a warm-up; device times by events over 20 back-to-back calls).  Pages: 16 of 1024 x 1024,
half photo-like and half flat (tests/png_encode_common.photo / flat_layout), and one 4096 x 4096 photo-like page.  Per set:
  file bytes of the stored and of the packed form (and Pillow's default level 6 for scale)
  host ms per item of __getitem__: mode='packed' and mode='device' on the packed archive, mode='raw' on the stored archive
  the inflate and the unfilter launch, us, next to the stored decode (gather + unfilter) of the same pages, re-measured in the same run
  the inflate launch as a share of the training step
Prints the figures and one JSON line (kept in profiles/page_inflate_bench.json).
usage: python tools/bench_page_inflate.py [--json PATH]"""
import io
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

import png_encode_common as E
from bench_page_decode import PASSES, STEP_MS, event_us, item_ms, write_zip
from layoutdetr_amd import repack_dataset
from layoutdetr_amd.training import dataset_layoutganpp as D


def pillow_level6_bytes(arr):
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(arr).save(buf, format='png')
    return len(buf.getvalue())


def bench(stored_zip, packed_zip, pages, size, dev):
    st = repack_dataset.repack(stored_zip, packed_zip, 'best')
    assert st['routes'] == {'raw': len(pages), 'decoded': 0}
    ds = dict(packed=D.LayoutDataset(path=packed_zip, background_size=size, mode='packed'), device=D.LayoutDataset(path=packed_zip, background_size=size, mode='device'),
              raw=D.LayoutDataset(path=stored_zip, background_size=size, mode='raw'))
    n = len(pages)
    row = dict(pages=n, side=int(pages[0].shape[0]), stored_bytes=st['bytes_before'], packed_bytes=st['bytes_after'], pillow_level6_bytes=sum(pillow_level6_bytes(p) for p in pages))
    row['packed_getitem_ms'] = item_ms(ds['packed'])
    row['device_getitem_ms'] = item_ms(ds['device'])
    row['raw_getitem_ms'] = item_ms(ds['raw'])
    packed = [ds['packed'][i][0]['background'] for i in range(n)]
    stored = [ds['raw'][i][0]['background'] for i in range(n)]
    row['packed_pages'] = sum(1 for p in packed if isinstance(p, D.RawPage) and p.kind == 'packed')     # (a page whose every segment stayed stored takes the stored path)
    assert all(isinstance(p, D.RawPage) for p in packed + stored)
    idx = [i for i, p in enumerate(packed) if p.kind == 'packed']
    want = torch.from_numpy(np.stack(pages))
    s_state, p_state = {}, {}
    assert torch.equal(D._decode_group(stored, dev, state=s_state).cpu(), want), 'the stored decode differs from the pixels'
    row['stored_gather_us'] = event_us(lambda: D._decode_group(stored, dev, phases=1, state=s_state))
    row['stored_unfilter_us'] = event_us(lambda: D._decode_group(stored, dev, phases=2, state=s_state))
    row['stored_decode_us'] = event_us(lambda: D._decode_group(stored, dev, phases=3, state=s_state))
    if idx:
        got, status = D._inflate_group([packed[i] for i in idx], dev, state=p_state)
        assert torch.equal(got.cpu(), want[idx]) and not status.cpu().any(), 'the inflate differs from the pixels'
        row['kinds'] = np.bincount(np.concatenate([packed[i].packed[0][:, 2] for i in idx]), minlength=3).tolist()      # segments stored / fixed / dynamic
        group = [packed[i] for i in idx]
        row['inflate_us'] = event_us(lambda: D._inflate_group(group, dev, phases=1, state=p_state))
        row['inflate_unfilter_us'] = event_us(lambda: D._inflate_group(group, dev, phases=2, state=p_state))
        row['inflate_decode_us'] = event_us(lambda: D._inflate_group(group, dev, phases=3, state=p_state))
        row['inflate_share_of_step'] = [row['inflate_us'] / 1e3 / s for s in STEP_MS]
        row['inflate_us_per_page_vs_host_ms'] = [row['inflate_us'] / len(idx), row['device_getitem_ms']]
    print(f"{n} x {row['side']}^2: stored {row['stored_bytes']} B, packed {row['packed_bytes']} B ({row['packed_bytes'] / row['stored_bytes']:.3f}; Pillow level 6: {row['pillow_level6_bytes']} B); "
          f"__getitem__ packed {row['packed_getitem_ms']:.3f} / device {row['device_getitem_ms']:.2f} / raw-on-stored {row['raw_getitem_ms']:.3f} ms per item; "
          f"stored decode {row['stored_decode_us']:.0f} us = gather {row['stored_gather_us']:.0f} + unfilter {row['stored_unfilter_us']:.0f}; "
          + (f"inflate {row['inflate_us']:.0f} us + unfilter {row['inflate_unfilter_us']:.0f} us = {row['inflate_decode_us']:.0f} us for {len(idx)} packed pages, "
             f"{100 * row['inflate_share_of_step'][0]:.2f} % of the step" if idx else 'no packed page'))
    for d in ds.values():
        d.close()
    return row


def main():
    out_path = sys.argv[sys.argv.index('--json') + 1] if '--json' in sys.argv else None
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        small = [E.photo(1024, 1024, seed=i) if i % 2 == 0 else E.flat_layout(1024, 1024, seed=i) for i in range(16)]
        big = [E.photo(4096, 4096, seed=99)]
        for name, pages in (('pages1024', small), ('page4096', big)):
            stored_zip, packed_zip = os.path.join(tmp, name + '_stored.zip'), os.path.join(tmp, name + '_packed.zip')
            write_zip(stored_zip, pages)
            rows.append(bench(stored_zip, packed_zip, pages, 1024, dev))
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), host_cpus=len(os.sched_getaffinity(0)), passes=PASSES, step_ms=STEP_MS, rows=rows))
    print(line)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
