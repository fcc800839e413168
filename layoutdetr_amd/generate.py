"""Layout generation: a background, a list of strings and their labels in, ranked layouts out -- the model call and the box post-processing of
the reference's `generate.py` (:299-329) and `generate_util.py::generate_banners` (:413-450), without their HTML / browser rendering.

The reference calls G once per seed (trunk at 1024 x 1024, BERT, six encoder layers, all identical for every seed), finishes the boxes with
Python double loops over 0-d device tensors and sorts on the host.  Here the condition is computed once (`Sampler.encode`), K candidates are
decoded against it (`Sampler.sample`, training/shared_decode.py) and all of them are finished, scored and ranked by one launch
(csrc/layout_finish.hip).  One `Condition` serves any number of `sample` calls: "the same banner, more variations" never re-runs the trunk.

    python -m layoutdetr_amd.generate --ckpt SNAPSHOT --bg IMG --strings 'a|b' --string-labels 'header|button' --seeds 1-5 --outfile X

Limits: 9 element slots per layout (the model's), K * 9 <= 16384 query rows per condition and call (decoded 128 candidates = 1152 rows per
condition and launch) and K <= 1024 candidates per finishing launch.
"""
import json
import math
import os
import re

import numpy as np
import torch

from .hip import core

NONE, CENTER, LEFT = 0, 1, 2
MODE_NAMES = {'none': NONE, 'horizontal_center_aligned': CENTER, 'horizontal_left_aligned': LEFT}
N_SLOTS = 9
MAX_CANDIDATES = 1024
# element types in label-index order (generate.py's label2index)
LABEL_LIST = ['header', 'pre-header', 'post-header', 'body', 'disclaimer / footnote', 'button', 'callout', 'logo']
# --bg-preprocessing, the reference's eight choices (generate.py:214)
BG_MODES = ['256', '128', 'blur', 'jpeg', 'rec', '3x_mask', 'edge', 'none']
# one colour per label for the box overlay (this package's own fixed palette)
PALETTE = [(230, 57, 70), (244, 162, 97), (233, 196, 106), (42, 157, 143), (38, 70, 83), (69, 123, 157), (131, 56, 236), (106, 153, 78)]


def _draws(seeds, draw):
    """draw(RandomState(seed)) per seed, stacked.  One generator object is re-seeded per seed: the stream is that of a fresh RandomState(seed),
    without the operating-system entropy a fresh object fetches before it is seeded (60 x the cost of the draw itself)."""
    rs = np.random.RandomState(0)
    out = []
    for s in seeds:
        rs.seed(int(s))
        out.append(draw(rs))
    return torch.from_numpy(np.concatenate(out)).to(torch.float32)


def latents(seeds, z_dim):
    """[K, 9, z_dim] fp32: row k is np.random.RandomState(seed_k).randn(1, 9, z_dim) cast to fp32 (generate_util.py:416)."""
    return _draws(seeds, lambda rs: rs.randn(1, N_SLOTS, z_dim))


def jitter_factors(seeds, strength=0.2):
    """[K, 9, 4] fp32: exp of RandomState(seed).uniform(log(1 - s), log(1 + s), (1, 9, 4)) cast to fp32, formed on the host with torch exactly as
    generate_util.py:145-148 / generate.py:88-91 form it, so the kernel only multiplies."""
    lo, hi = math.log(1.0 - strength), math.log(1.0 + strength)
    return _draws(seeds, lambda rs: rs.uniform(low=lo, high=hi, size=(1, N_SLOTS, 4))).exp()


def reference_plan(seeds, post_process, rng=None):
    """Per candidate (jitter: bool, mode in {CENTER, LEFT}), drawn in the order of generate_util.py:424-433 from `rng` (an object with .rand():
    np.random itself, the reference's source, by default, or a RandomState).  The reference's short-circuits apply: seed 1 draws no jitter
    number, and a key missing from `post_process` draws nothing."""
    rng = np.random if rng is None else rng
    plan = []
    for seed in seeds:
        jit = bool(int(seed) != 1 and 'jitter' in post_process and rng.rand() < post_process['jitter'])
        center = bool('horizontal_center_aligned' in post_process and rng.rand() < post_process['horizontal_center_aligned'])
        plan.append((jit, CENTER if center else LEFT))
    return plan


def parse_range(s):
    """'1,3-5' -> [1, 3, 4, 5] (generate.py's --seeds syntax)."""
    if isinstance(s, (list, tuple)):
        return [int(v) for v in s]
    out = []
    for part in str(s).split(','):
        m = re.match(r'^\s*(\d+)\s*-\s*(\d+)\s*$', part)
        if m:
            out.extend(range(int(m.group(1)), int(m.group(2)) + 1))
        else:
            out.append(int(part))
    return out


def parse_labels(s):
    """'header|button' -> [0, 5]; an unknown name is an error that lists the known ones."""
    names = s.split('|') if isinstance(s, str) else list(s)
    out = []
    for n in names:
        if n not in LABEL_LIST:
            raise ValueError(f'unknown label {n!r}: one of {LABEL_LIST}')
        out.append(LABEL_LIST.index(n))
    return out


def resolve_background(bg, mode):
    """(background path, --bg-preprocessing mode) -> (path of the image the model sees, page_filter, size it is resized to), generate.py:263-284:
    '256' / '128' resize the page to that size instead of 1024; 'blur' / 'edge' filter the page on the device (filter_pages) before the resize
    to 1024; 'jpeg' reads <dir>_jpeg/<name with .png -> .jpg> and 'rec' <dir>_rec/<name>, siblings of the page's directory (:270-279; a bare
    file name counts as lying in the current directory); '3x_mask' and 'none' take the page as it is.  A missing sibling file is an error
    that names the path looked for.  No GPU work."""
    if mode not in BG_MODES:
        raise ValueError(f'unknown background preprocessing {mode!r}: one of {BG_MODES}')
    if mode in ('256', '128'):
        return bg, None, int(mode)
    if mode in ('blur', 'edge'):
        return bg, mode, 1024
    if mode in ('jpeg', 'rec'):
        d, name = os.path.split(bg)
        d = (d or os.getcwd()).rstrip('/')
        path = os.path.join(d + '_' + mode, name.replace('.png', '.jpg') if mode == 'jpeg' else name)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"--bg-preprocessing {mode}: {path} not found (the {mode} version of {bg} is looked for in the sibling directory '<dir>_{mode}')")
        return path, None, 1024
    return bg, None, 1024


def layout_finish(bbox, num, factors=None, jitter=None, modes=None):
    """csrc/layout_finish.hip on bbox [C, K, N, 4]: num [C, K] int32 valid prefix lengths, factors [C, K, N, 4] or None, jitter [C, K] uint8 or
    None, modes [C, K] uint8 (None: NONE everywhere) -> (bbox_out, overlap [C, K], alignment [C, K], order [C, K] int32)."""
    core.require_gpu(bbox, num, factors, jitter, modes)
    if bbox.ndim != 4 or bbox.shape[-1] != 4:
        raise ValueError(f'layout_finish: bbox must be [C, K, N, 4] (got {tuple(bbox.shape)})')
    C, K, N, _ = bbox.shape
    dev = bbox.device
    bbox = core.f32c(bbox)
    num = num.to(torch.int32).expand(C, K).contiguous() if num.ndim == 2 else num.to(torch.int32).view(C, 1).expand(C, K).contiguous()
    modes = torch.zeros((C, K), dtype=torch.uint8, device=dev) if modes is None else modes.to(torch.uint8).expand(C, K).contiguous()
    if factors is not None:
        factors = core.f32c(factors.expand(C, K, N, 4))
    if jitter is not None:
        jitter = jitter.to(torch.uint8).expand(C, K).contiguous()
    out = torch.empty_like(bbox)
    overlap = torch.empty((C, K), dtype=torch.float32, device=dev)
    alignment = torch.empty((C, K), dtype=torch.float32, device=dev)
    order = torch.empty((C, K), dtype=torch.int32, device=dev)
    core.check(core.lib().ldetr_layout_finish_f32(core.ptr(bbox), core.ptr(num), core.ptr(factors), core.ptr(jitter), core.ptr(modes), core.ptr(out),
                                                  core.ptr(overlap), core.ptr(alignment), core.ptr(order), C, K, N, core.stream()), 'layout_finish')
    return out, overlap, alignment, order


class Layouts(object):
    """Result of `Sampler.sample`: bbox_raw, bbox [C, K, 9, 4] (xc, yc, w, h; the generator's output and the finished boxes), overlap, alignment,
    order [C, K] (order[c]: candidate indices ascending by overlap, stable), num [C] valid elements per condition, and the plan that was applied
    (jitter [K] bool, modes [K])."""

    def __init__(self, bbox_raw, bbox, overlap, alignment, order, num, jitter, modes, seeds=None):
        self.bbox_raw, self.bbox, self.overlap, self.alignment, self.order = bbox_raw, bbox, overlap, alignment, order
        self.num, self.jitter, self.modes, self.seeds = num, jitter, modes, seeds

    def sheet(self, page_u8, labels, canvas=256, nrow=None, condition=0):
        """Contact sheet of one condition: its K candidates in rank order (best first), each drawn over the page, as ONE raster launch with one
        shared page (render.layout_grid: the drawing rule of the training snapshots, this module's palette).  page_u8: uint8 [H, W, 3];
        labels: the condition's label indices, one per element.  -> uint8 [Hg, Wg, 3] on the boxes' device."""
        from . import render
        labels = [int(l) % len(PALETTE) for l in labels]
        n = len(labels)
        if not 1 <= n <= N_SLOTS:
            raise ValueError(f'sheet: 1..{N_SLOTS} labels, one per element')
        dev = self.bbox.device
        K = self.bbox.shape[1]
        boxes = self.bbox[condition].index_select(0, self.order[condition].long())          # rank order, no host round trip
        valid = (torch.arange(N_SLOTS) < n).expand(K, N_SLOTS)
        lab = torch.tensor(labels + [0] * (N_SLOTS - n), dtype=torch.int32).expand(K, N_SLOTS)
        page = torch.as_tensor(page_u8).to(dev)
        if page.dtype != torch.uint8 or page.ndim != 3 or page.shape[2] != 3:
            raise ValueError('sheet: the page must be uint8 [H, W, 3]')
        return render.layout_grid(boxes, valid, lab, PALETTE, (int(page.shape[1]), int(page.shape[0])), pages=render.PageSet(page),
                                  page_index=[0] * K, canvas=canvas, nrow=nrow)


def _plan_arrays(K, jitter, modes):
    j = [False] * K if jitter is None else [bool(v) for v in jitter]
    m = [NONE] * K if modes is None else [int(v) for v in modes]
    if len(j) != K or len(m) != K or any(v not in (NONE, CENTER, LEFT) for v in m):
        raise ValueError(f'jitter / modes: one flag and one mode in (NONE, CENTER, LEFT) per candidate ({K})')
    return j, m


class Sampler(object):
    """Holds a Generator in eval mode with gradients off."""

    def __init__(self, G):
        self.G = G.eval().requires_grad_(False)

    @property
    def device(self):
        return next(self.G.parameters()).device

    def encode(self, background, texts_or_features, labels, padding_mask=None, background_size=None, page_filter=None):
        """background: [C, 3, S, S] normalised fp32, or uint8 pages [C, H, W, 3] / a list of [H, W, 3] pages of any size (resized to
        `background_size`, default 1024 as generate.py:284, and normalised on the device).  texts_or_features: per condition a list of up to 9
        strings (needs the module's tokenizer), or TextTokens / TextFeatures already padded to 9 slots.  labels: per condition a list of label
        indices, or a [C, 9] tensor.  padding_mask ([C, 9] bool, True = padded) defaults to the prefix mask of the list lengths.
        page_filter ('blur' / 'edge', uint8 pages only): the pages are filtered on the device before the resize (generate.py:267-269, 280-282)."""
        from .training.dataset_layoutganpp import background_to_tensor
        from .training.shared_decode import check_prefix_mask
        if padding_mask is not None:
            check_prefix_mask(torch.as_tensor(padding_mask))
        dev = self.device
        if isinstance(background, (list, tuple)):
            background = torch.stack([background_to_tensor(torch.as_tensor(p).to(dev), background_size or 1024, page_filter=page_filter) for p in background])
        elif background.dtype == torch.uint8:
            background = background_to_tensor(background.to(dev), background_size or 1024, page_filter=page_filter)
        elif page_filter is not None:
            raise ValueError('encode: page_filter needs uint8 pages, not an already normalised background')
        background = background.to(device=dev, dtype=torch.float32)
        C = background.shape[0]
        lens = None
        if isinstance(texts_or_features, (list, tuple)):
            if len(texts_or_features) != C or any(len(t) > N_SLOTS for t in texts_or_features):
                raise ValueError(f'texts: one list of at most {N_SLOTS} strings per condition ({C})')
            lens = [len(t) for t in texts_or_features]
            texts_or_features = [list(t) + [''] * (N_SLOTS - len(t)) for t in texts_or_features]      # generate_util.py:419
        if not torch.is_tensor(labels):
            if len(labels) != C or (lens is not None and [len(l) for l in labels] != lens):
                raise ValueError('labels: one label per string')
            lens = [len(l) for l in labels] if lens is None else lens
            labels = torch.tensor([list(l) + [0] * (N_SLOTS - len(l)) for l in labels], dtype=torch.int64)      # generate_util.py:422
        labels = labels.to(device=dev, dtype=torch.int64)
        if padding_mask is None:
            if lens is None:
                raise ValueError('padding_mask is needed when neither the texts nor the labels are lists')
            padding_mask = torch.arange(N_SLOTS)[None, :] >= torch.tensor(lens)[:, None]
        if tuple(labels.shape) != (C, N_SLOTS) or tuple(padding_mask.shape) != (C, N_SLOTS):
            raise ValueError(f'labels and padding_mask must be [{C}, {N_SLOTS}]')
        return self.G.encode_condition(background, labels, texts_or_features, padding_mask.to(dev))

    def sample(self, cond, seeds=None, z=None, jitter=None, modes=None, strength=0.2):
        """K candidates per condition from seeds (latents / jitter factors as the reference draws them) or from explicit z [K, 9, z_dim] /
        [C, K, 9, z_dim]; jitter: K flags (needs seeds), modes: K of NONE / CENTER / LEFT -- e.g. from reference_plan()."""
        if (seeds is None) == (z is None):
            raise ValueError('sample: pass seeds or z')
        dev = cond.device
        if seeds is not None:
            seeds = [int(s) for s in seeds]
            if not seeds:
                raise ValueError('sample: at least one seed')
            z = latents(seeds, self.G.z_dim)
        K = z.shape[-3]
        if K < 1 or K > MAX_CANDIDATES:
            raise ValueError(f'sample: 1 <= K <= {MAX_CANDIDATES} candidates per call (got {K})')
        jit, mod = _plan_arrays(K, jitter, modes)
        if any(jit) and seeds is None:
            raise ValueError('sample: jitter needs seeds (the factors are drawn from them)')
        bbox_raw = self.G.decode_candidates(cond, z.to(dev))
        factors = jitter_factors(seeds, strength).to(dev).unsqueeze(0) if any(jit) else None
        jflags = torch.tensor(jit, dtype=torch.uint8).to(dev).unsqueeze(0) if any(jit) else None
        mflags = torch.tensor(mod, dtype=torch.uint8).to(dev).unsqueeze(0)
        bbox, overlap, alignment, order = layout_finish(bbox_raw, cond.num, factors, jflags, mflags)
        return Layouts(bbox_raw, bbox, overlap, alignment, order, cond.num, jit, mod, seeds)


def generate_layouts(G, background, texts, labels, seeds, post_process=None, rng=None, strength=0.2, background_size=None, page_filter=None):
    """The one-call form.  post_process: None (no finishing), a dict of probabilities as generate_banners takes it (drawn by reference_plan from
    `rng`), or a list of (jitter, mode) per seed."""
    s = Sampler(G)
    cond = s.encode(background, texts, labels, background_size=background_size, page_filter=page_filter)
    seeds = list(seeds)
    if post_process is None:
        plan = [(False, NONE)] * len(seeds)
    elif isinstance(post_process, dict):
        plan = reference_plan(seeds, post_process, rng)
    else:
        plan = list(post_process)
    return s.sample(cond, seeds=seeds, jitter=[p[0] for p in plan], modes=[p[1] for p in plan], strength=strength)


# ---------------------------------------------------------------------------------------------------------------------------------
# command line


def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog='python -m layoutdetr_amd.generate', description=__doc__.split('\n\n')[0])
    p.add_argument('--ckpt', '--network', dest='ckpt', required=True, help='snapshot written by training_loop.save_snapshot')
    p.add_argument('--bg', required=True, help='background image')
    p.add_argument('--bg-preprocessing', default='none', choices=BG_MODES,
                   help="256 / 128: resize the page to that size instead of 1024; blur / edge: Gaussian blur (radius 3) / grey edge filter on the device, then "
                        "resize to 1024; jpeg / rec: read <dir>_jpeg/<name>.jpg / <dir>_rec/<name> instead of the page; 3x_mask: the same as none (as in the reference)")
    p.add_argument('--strings', required=True, help="texts separated by '|'")
    p.add_argument('--string-labels', required=True, help="one label per text separated by '|': " + ', '.join(LABEL_LIST))
    p.add_argument('--seeds', type=parse_range, default=[0], help="e.g. '1,3-5'")
    p.add_argument('--out-postprocessing', default='none', choices=sorted(MODE_NAMES))
    p.add_argument('--out-jittering-strength', type=float, default=0.0)
    p.add_argument('--vocab', default=None, help='bert-base-uncased vocab.txt when the snapshot does not carry a tokenizer (or set LDETR_BERT_VOCAB)')
    p.add_argument('--sheet', action='store_true', help='also write <outfile>_sheet.png: every candidate over the page, in rank order')
    p.add_argument('--outfile', required=True)
    return p


def parse_args(argv=None):
    a = build_parser().parse_args(argv)
    a.texts = a.strings.split('|')
    a.labels = parse_labels(a.string_labels)
    if len(a.texts) != len(a.labels) or not 1 <= len(a.texts) <= N_SLOTS:
        raise ValueError(f'--strings and --string-labels: the same number (1..{N_SLOTS}) of entries')
    if not 0.0 <= a.out_jittering_strength < 1.0:
        raise ValueError('--out-jittering-strength must be in [0, 1)')
    a.mode = MODE_NAMES[a.out_postprocessing]
    return a


def load_generator(path, device, vocab=None):
    """G_ema (else G) of a snapshot, read as training_loop.load_resume reads it.  A save_snapshot pickle holds the modules and is all that is
    needed; a torch file of state dicts carries no architecture: build the Generator and fill it with training_loop.load_resume instead."""
    from .training.training_loop import read_snapshot
    data = read_snapshot(path)
    G = data.get('G_ema') if data.get('G_ema') is not None else data.get('G')
    if isinstance(G, dict):
        raise RuntimeError(f'{path}: holds state dicts, which do not say how to build the Generator; construct it and call training_loop.load_resume')
    if not isinstance(G, torch.nn.Module):
        raise RuntimeError(f'{path}: no G_ema / G module inside (expected a snapshot written by training_loop.save_snapshot)')
    if getattr(G, 'tokenizer', None) is None:
        from .training.networks_detr import _build_tokenizer
        G.tokenizer = _build_tokenizer(vocab)
    return G.to(device)


def draw_boxes(page, boxes, labels, path):
    """The page with the valid boxes drawn over it, largest first (as generate.py:67-84, with this package's palette)."""
    from PIL import ImageDraw
    img = page.convert('RGB').copy()
    W, H = img.size
    draw = ImageDraw.Draw(img, 'RGBA')
    for i in sorted(range(len(boxes)), key=lambda i: boxes[i][2] * boxes[i][3], reverse=True):
        xc, yc, w, h = [float(v) for v in boxes[i]]
        x1, x2 = sorted(((xc - w / 2) * W, (xc + w / 2) * W))
        y1, y2 = sorted(((yc - h / 2) * H, (yc + h / 2) * H))
        color = PALETTE[int(labels[i]) % len(PALETTE)]
        draw.rectangle([x1, y1, x2, y2], outline=color, fill=color + (100,))
    img.save(path, format='png')


def main(argv=None):
    import PIL.Image
    a = parse_args(argv)
    path, page_filter, size = resolve_background(a.bg, a.bg_preprocessing)
    dev = torch.device('cuda')
    G = load_generator(a.ckpt, dev, a.vocab)
    page = PIL.Image.open(a.bg).convert('RGB')                     # what the boxes are drawn over: always the original page (generate.py:252)
    seen = page if path == a.bg else PIL.Image.open(path).convert('RGB')
    s = Sampler(G)
    cond = s.encode([torch.from_numpy(np.array(seen))], [a.texts], [a.labels], background_size=size, page_filter=page_filter)
    K = len(a.seeds)
    res = s.sample(cond, seeds=a.seeds, jitter=[a.out_jittering_strength > 0.0] * K, modes=[a.mode] * K, strength=a.out_jittering_strength or 0.2)
    n = len(a.texts)
    order = res.order[0].tolist()
    out = dict(strings=a.texts, labels=[LABEL_LIST[l] for l in a.labels], seeds=a.seeds, order=order,
               plan=[dict(seed=sd, jitter=bool(j), mode=[k for k, v in MODE_NAMES.items() if v == m][0]) for sd, j, m in zip(a.seeds, res.jitter, res.modes)],
               overlap=res.overlap[0].tolist(), alignment=res.alignment[0].tolist(), bbox=res.bbox[0, :, :n].tolist(), bbox_raw=res.bbox_raw[0, :, :n].tolist())
    os.makedirs(os.path.dirname(os.path.abspath(a.outfile)), exist_ok=True)
    with open(a.outfile + '.json', 'w') as f:
        json.dump(out, f, indent=1)
    draw_boxes(page, res.bbox[0, order[0], :n].tolist(), a.labels, a.outfile + '_bboxes.png')
    if a.sheet:
        from . import render
        render.save_png(res.sheet(torch.from_numpy(np.array(page)), a.labels), a.outfile + '_sheet.png')
    print(f'wrote {a.outfile}.json and {a.outfile}_bboxes.png' + (f' and {a.outfile}_sheet.png' if a.sheet else '') + f' (best candidate: seed {a.seeds[order[0]]}, overlap {out["overlap"][order[0]]:.4f})')


if __name__ == '__main__':
    main()
