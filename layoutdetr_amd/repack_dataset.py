"""Repack a dataset archive once so that its page backgrounds are decoded on the GPU from COMPRESSED files:

    python -m layoutdetr_amd.repack_dataset SRC.zip DST.zip [--blocks best|stored]

Every page PNG entry (`<base>_background_orig.png`) is decoded -- on the device where `scan_png` finds it eligible (a stored-block file, what the
reference's dataset_tool.py writes), else with Pillow --, re-encoded on the device with `render.encode_png(index=True)` and written ZIP_STORED under the
same name; every other entry is copied byte for byte.  The result is still a valid PNG-in-zip archive: the reference, mode='device' and mode='raw' read it
(decoders skip the ancillary ldIX chunk), and `LayoutDataset(mode='packed')` inflates the indexed pages on the GPU.  --blocks best (default) takes the
smallest of a stored, fixed and dynamic block per 64 KiB segment; --blocks stored writes stored blocks only (the files mode='raw' already takes).
Prints the page bytes before and after and the route counts.  Needs a GPU: the encoder has no CPU path."""
import argparse
import io
import sys
import zipfile

import numpy as np

PAGE_SUFFIX = '_background_orig.png'
BLOCKS = {'best': 'auto', 'stored': 'stored'}                              # --blocks -> render.encode_png(blocks=...)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog='python -m layoutdetr_amd.repack_dataset', description='Re-encode the page PNGs of a dataset archive with the device encoder and its index chunk.')
    ap.add_argument('src', metavar='SRC.zip')
    ap.add_argument('dst', metavar='DST.zip')
    ap.add_argument('--blocks', choices=sorted(BLOCKS), default='best', help="'best': the smallest block type per segment (default); 'stored': stored blocks only")
    args = ap.parse_args(argv)
    if args.src == args.dst:
        ap.error('SRC and DST must differ')
    return args


def is_page(name):
    return name.endswith(PAGE_SUFFIX)


def _decode_page(data, device):
    """(uint8 [H, W, 3] on the device, 'raw' | 'decoded')."""
    import torch
    from .training.dataset_layoutganpp import decode_pages, scan_png
    raw = scan_png(data)
    if raw is not None:
        return decode_pages([raw], device)[0], 'raw'
    import PIL.Image
    page = np.array(PIL.Image.open(io.BytesIO(data)))
    if page.ndim != 3 or page.shape[2] != 3:
        raise ValueError('expected an RGB page')
    return torch.from_numpy(np.ascontiguousarray(page)).to(device), 'decoded'


def _device_recode(data, blocks):
    import torch
    from . import render
    page, route = _decode_page(data, torch.device('cuda'))
    return render.encode_png(page, blocks=BLOCKS[blocks], index=True).numpy().tobytes(), route


def repack(src, dst, blocks='best', recode=None):
    """Copy the archive `src` to `dst`, page PNGs re-encoded by recode(file bytes, blocks) -> (new file bytes, route) (default: decode + encode on the
    device).  Returns dict(pages, bytes_before, bytes_after, routes)."""
    recode = _device_recode if recode is None else recode
    stats = dict(pages=0, bytes_before=0, bytes_after=0, routes={'raw': 0, 'decoded': 0})
    with zipfile.ZipFile(src) as zin, zipfile.ZipFile(dst, 'w') as zout:
        for info in zin.infolist():
            data = zin.read(info.filename)
            if not is_page(info.filename):
                zout.writestr(info, data, compress_type=info.compress_type)
                continue
            try:
                new, route = recode(data, blocks)
            except Exception as e:
                raise ValueError(f'{src}: {info.filename}: {e}') from e
            zout.writestr(info.filename, new, compress_type=zipfile.ZIP_STORED)
            stats['pages'] += 1
            stats['bytes_before'] += len(data)
            stats['bytes_after'] += len(new)
            stats['routes'][route] += 1
    return stats


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    st = repack(args.src, args.dst, args.blocks)
    ratio = st['bytes_after'] / st['bytes_before'] if st['bytes_before'] else 0.0
    print(f"{st['pages']} page PNGs: {st['bytes_before']} bytes -> {st['bytes_after']} bytes ({ratio:.3f}); decoded on the device (stored blocks): {st['routes']['raw']}, "
          f"with Pillow: {st['routes']['decoded']}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
