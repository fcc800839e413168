"""Stored-block PNG pages decoded on the device (csrc/png_decode.hip) against live Pillow, exact equality everywhere: the kernels over the size x
filter schedule x block / chunk layout grid of tests/png_decode_common.py, a batch in one call, Pillow-written files, the dataset route
(mode='raw' -> collate -> batch_backgrounds_to_device -> assemble_batch) against the mode='device' route, and the entry's refusals."""
import ctypes
import io
import os
import zipfile

import numpy as np
import pytest
import torch

import png_decode_common as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZIP = os.path.join(ROOT, 'tests', 'golden', 'dataset_tiny.zip')


def _decode(dev, files):
    from layoutdetr_amd.training.dataset_layoutganpp import decode_pages, scan_png
    raws = [scan_png(f) for f in files]
    assert all(r is not None for r in raws)
    return decode_pages(raws, dev)


@pytest.mark.parametrize('sched', P.SCHEDULE_NAMES)
@pytest.mark.parametrize('wh', P.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_decode_equals_pillow(dev, wh, sched):
    """One noise page per (size, schedule), written in the five block / chunk layouts and decoded in one call."""
    W, H = wh
    px, files = P.case_files(W, H, sched)
    names = list(files)
    got = _decode(dev, [files[k] for k in names]).cpu().numpy()
    assert got.shape == (len(names), H, W, 3) and got.dtype == np.uint8
    for i, k in enumerate(names):
        want = P.pillow_decode(files[k])
        bad = int((got[i] != want).sum())
        print(f'{W}x{H} {sched} {k}: {bad} bytes differ')
        assert np.array_equal(want, px), k                     # (the writer, as in the CPU test)
        assert np.array_equal(got[i], want), k


def test_three_pages_in_one_call_equal_each_alone(dev):
    W, H = 65, 130
    combos = [('all_4', 'pillow_65535_65536'), ('random_mix', 'blocks_0_5_1_0_17_chunks_1_2_7_4'), ('row0_1_then_3', 'ancillary')]
    files = [P.write_stored_png(P.noise_page(W, H, 40 + i), P.schedules(H, i)[s], **P.LAYOUTS[l]) for i, (s, l) in enumerate(combos)]
    got = _decode(dev, files)
    assert got.shape == (3, H, W, 3)
    for i, f in enumerate(files):
        assert torch.equal(_decode(dev, [f])[0], got[i]), i
        assert np.array_equal(got[i].cpu().numpy(), P.pillow_decode(f)), i


def test_pages_of_two_sizes_come_back_as_a_list_in_order(dev):
    files = [P.case_files(7, 7, 'all_4')[1]['ancillary'], P.case_files(2, 3, 'all_3')[1]['blocks_1_chunks_3'], P.case_files(7, 7, 'all_1')[1]['one_block_one_chunk']]
    got = _decode(dev, files)
    assert isinstance(got, list) and [tuple(g.shape) for g in got] == [(7, 7, 3), (3, 2, 3), (7, 7, 3)]
    for g, f in zip(got, files):
        assert np.array_equal(g.cpu().numpy(), P.pillow_decode(f))


def _pil_bytes(arr):
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(arr).save(buf, format='png', compress_level=0, optimize=False)       # dataset_tool.py:325-363
    return buf.getvalue()


def test_fixture_pages(dev):
    with zipfile.ZipFile(ZIP) as z:
        files = [z.read(n) for n in sorted(z.namelist()) if n.endswith('_background_orig.png')]
    assert len(files) == 3
    got = _decode(dev, files).cpu().numpy()
    for i, f in enumerate(files):
        assert np.array_equal(got[i], P.pillow_decode(f)), i


def test_pillow_written_1024_page(dev):
    """Smooth content with noise on top: Pillow picks several filter types, 94 stored blocks in 49 IDAT chunks."""
    yy, xx = np.mgrid[0:1024, 0:1024]
    page = np.stack([(xx // 4) % 256, (yy // 4) % 256, ((xx + yy) // 8) % 256], -1).astype(np.uint8)
    page[256:768] ^= np.random.RandomState(0).randint(0, 8, size=(512, 1024, 3)).astype(np.uint8)
    page[900:] = np.random.RandomState(1).randint(0, 256, size=(124, 1024, 3)).astype(np.uint8)
    f = _pil_bytes(page)
    got = _decode(dev, [f])
    assert torch.equal(got[0].cpu(), torch.from_numpy(P.pillow_decode(f)))
    assert np.array_equal(got[0].cpu().numpy(), page)


# ---------------------------------------------------------------------------------------------------------------------------------
# the dataset route


def _route(dev, path, mode, page_filter=None):
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset, batch_backgrounds_to_device
    ds = LayoutDataset(path=path, background_size=32, mode=mode)
    samples, labels = LayoutDataset.collate([ds[i] for i in range(len(ds))])
    return ds, samples, labels, batch_backgrounds_to_device(samples['background'], 32, dev, page_filter=page_filter)


@pytest.mark.parametrize('page_filter', [None, 'blur'])
def test_raw_route_equals_device_route_on_the_fixture(dev, page_filter):
    ds, _, _, raw = _route(dev, ZIP, 'raw', page_filter)
    _, _, _, ref = _route(dev, ZIP, 'device', page_filter)
    assert ds.route_counts == {'raw': 3, 'decoded': 0}
    assert raw.shape == (3, 3, 32, 32) and raw.dtype == torch.float32 and torch.equal(raw, ref)


def test_mixed_batch_one_item_falls_back(dev, tmp_path):
    import PIL.Image
    path = str(tmp_path / 'mixed.zip')
    with zipfile.ZipFile(ZIP) as src, zipfile.ZipFile(path, 'w', zipfile.ZIP_STORED) as out:
        pages = sorted(n for n in src.namelist() if n.endswith('_background_orig.png'))
        for n in src.namelist():
            data = src.read(n)
            if n == pages[1]:                                  # smooth it, so that level 6 really compresses
                im = PIL.Image.open(io.BytesIO(data)).convert('RGB').resize((8, 6)).resize((80, 56))
                buf = io.BytesIO()
                im.save(buf, format='png', compress_level=6)
                data = buf.getvalue()
            out.writestr(n, data)
    ds, samples, _, raw = _route(dev, path, 'raw')
    _, _, _, ref = _route(dev, path, 'device')
    assert ds.route_counts == {'raw': 2, 'decoded': 1}
    assert sum(torch.is_tensor(p) for p in samples['background']) == 1
    assert torch.equal(raw, ref)


def test_assemble_batch_background_equal_under_both_modes(dev):
    from layoutdetr_amd.training.training_loop import assemble_batch
    out = {}
    for mode in ('device', 'raw'):
        _, samples, labels, _ = _route(dev, ZIP, mode)
        out[mode] = assemble_batch(samples, labels, object(), 32, dev)
    assert torch.equal(out['raw']['background'], out['device']['background'])
    for k in ('bbox_real', 'bbox_class', 'padding_mask', 'real_c'):
        assert torch.equal(out['raw'][k], out['device'][k]), k


def test_raw_batch_through_a_pinning_dataloader(dev):
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset, RawPage, batch_backgrounds_to_device
    ds = LayoutDataset(path=ZIP, background_size=32, mode='raw')
    # (the backgrounds alone: torch cannot pin the 0-stride 'patches' placeholder of a whole batch, in 'device' mode either)
    loader = torch.utils.data.DataLoader(ds, batch_size=3, collate_fn=lambda items: {'background': ds.collate(items)[0]['background']}, pin_memory=True)
    pages = next(iter(loader))['background']
    assert all(isinstance(p, RawPage) and p.tensor().is_pinned() for p in pages)
    assert torch.equal(batch_backgrounds_to_device(pages, 32, dev), _route(dev, ZIP, 'device')[3])


# ---------------------------------------------------------------------------------------------------------------------------------
# the entry refuses bad host tables without launching


def _args(dev, raw, seg=None, jobs=None):
    from layoutdetr_amd import _lib
    from layoutdetr_amd.training import dataset_layoutganpp as D
    off, s, j, nbytes = D._png_tables([raw])
    s = s if seg is None else seg
    j = j if jobs is None else jobs
    files = torch.zeros(nbytes, dtype=torch.uint8)
    files[:raw.data.size] = torch.from_numpy(raw.data)
    H, W = raw.height, raw.width
    keep = dict(files=files.to(dev), off=torch.from_numpy(off).to(dev), seg=torch.from_numpy(s).to(dev), jobs=torch.from_numpy(j).to(dev),
                scratch=torch.zeros((H * (1 + 3 * W) + 15) // 16 * 16, dtype=torch.uint8, device=dev),
                dst=torch.full((1, H, W, 3), 7, dtype=torch.uint8, device=dev), host=(off, s, j))
    a = _lib.PngDecodeArgs(struct_bytes=ctypes.sizeof(_lib.PngDecodeArgs), n=1, H=H, W=W, phases=3, reserved=0, files=keep['files'].data_ptr(),
                           files_bytes=nbytes, file_off=off.ctypes.data, file_off_dev=keep['off'].data_ptr(), segments=s.ctypes.data,
                           segments_dev=keep['seg'].data_ptr(), n_segments=len(s), jobs=j.ctypes.data, jobs_dev=keep['jobs'].data_ptr(), n_jobs=len(j),
                           scratch=keep['scratch'].data_ptr(), scratch_bytes=keep['scratch'].numel(), dst=keep['dst'].data_ptr())
    return a, keep


def test_entry_refuses_bad_tables_without_launching(dev):
    from layoutdetr_amd.hip import core
    from layoutdetr_amd.training import dataset_layoutganpp as D
    px, files = P.case_files(7, 7, 'random_mix')
    raw = D.scan_png(files['blocks_0_5_1_0_17_chunks_1_2_7_4'])
    lib = core.lib()
    _, good_seg, good_jobs, nbytes = D._png_tables([raw])

    def run(seg=None, jobs=None):
        a, keep = _args(dev, raw, seg, jobs)
        rc = lib.ldetr_png_decode_u8(ctypes.byref(a), core.stream())
        torch.cuda.synchronize()
        return rc, lib.ldetr_last_error().decode(), keep

    rc, _, keep = run()
    assert rc == 0 and np.array_equal(keep['dst'][0].cpu().numpy(), px)
    leaves = good_seg.copy(); leaves[3, 1] = nbytes                              # a segment that reaches past the end of its (16-byte padded) file
    gap = good_seg.copy(); gap[2, 2] += 1                                        # stream offsets that leave a hole
    short = good_seg[:-1].copy()                                                 # the stream is not covered to its end
    rows = good_jobs.copy(); rows[-1, 2] -= 1                                    # the row ranges stop one row early
    for name, kw, word in (('leaves', dict(seg=leaves), 'leaves its file'), ('gap', dict(seg=gap), 'does not continue'), ('short', dict(seg=short), 'do not tile'),
                           ('rows', dict(jobs=rows), 'row range')):
        rc, msg, keep = run(**kw)
        assert rc == 1 and word in msg, (name, rc, msg)
        assert bool((keep['dst'] == 7).all()) and bool((keep['scratch'] == 0).all()), name     # nothing was launched
