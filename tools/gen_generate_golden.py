"""Generates tests/golden/generate.npz by driving the REFERENCE (salesforce/LayoutDETR) on the CPU: data only.

Run where the reference tree is available:  python tools/gen_generate_golden.py [path to the reference]
Stored: 256 seeded layouts pushed through the reference's own finishing functions (generate_util.py: jitter :145-148,
horizontal_center_aligned :100-103, horizontal_left_aligned :105-115, de_overlap :117-141) and compute_overlap / compute_alignment
(metrics/metric_layoutnet.py:153-201), in fp32 AND in fp64.  de_overlap branches on `abs(yc2 - yc1) < h1/2 + h2/2` and `yc1 < yc2`, which are
discontinuous: a case whose fp32 and fp64 runs disagree pins nothing and is dropped (at most 10 % may be).  Also stored, the draws of a few
seeds: the jitter factors come from the reference's jitter() itself (applied to ones); the latents (generate_util.py:416) and the jitter /
alignment decisions for seeds 1..8 under np.random.seed(0) with the server's probabilities (:424-433) are RESTATED here, because they sit
inline in generate_banners, which cannot run without a browser.  Those two pin the package's functions against an independent statement of the
numpy draw order (which seeds, which distribution, which draw a short-circuit skips), not against a run of the reference.  Modules the
reference cannot import here are stubbed as in oracle/gen_golden.py; none of the stubs takes part in a captured computation."""
import math
import os
import sys
import types

import numpy as np
import PIL.Image
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF as _DEFAULT_REF  # noqa: E402  (the one place that names where the reference tree lies)

REF = sys.argv[1] if len(sys.argv) > 1 else _DEFAULT_REF
OUT = os.path.join(ROOT, 'tests', 'golden', 'generate.npz')
N_CASES, N_SLOTS = 256, 9
BOX_TOL, METRIC_RTOL, METRIC_ATOL = 1e-5, 1e-5, 1e-6
MAX_DROPPED = 0.10
PLAN_PROBS = {'jitter': 5.0 / 6.0, 'horizontal_center_aligned': 2.0 / 3.0}


def _setup():
    sys.path.insert(0, REF)
    from oracle.gen_golden import _stub_modules
    _stub_modules()
    for name in ('seaborn', 'bs4', 'selenium', 'selenium.webdriver', 'metrics.rendering_utils'):
        sys.modules[name] = types.ModuleType(name)
    sys.modules['bs4'].BeautifulSoup = object
    sys.modules['selenium'].webdriver = sys.modules['selenium.webdriver']
    sys.modules['selenium.webdriver'].Chrome = object
    if not hasattr(np, 'bool'):
        np.bool = bool
    if not hasattr(PIL.Image, 'ANTIALIAS'):
        PIL.Image.ANTIALIAS = PIL.Image.LANCZOS


def run_case(gu, metrics, bbox, num, jitter, mode, seed, dtype):
    """One layout through the reference's functions in `dtype` -> (finished boxes [9, 4], overlap, alignment)."""
    b = bbox.clone().to(dtype).unsqueeze(0)
    mask = (torch.arange(N_SLOTS) < num).unsqueeze(0)
    if jitter:
        b = gu.jitter(b, seed)
    if mode == 1:
        b = gu.de_overlap(gu.horizontal_center_aligned(b, mask), mask)
    elif mode == 2:
        b = gu.de_overlap(gu.horizontal_left_aligned(b, mask), mask)
    return b[0], metrics.compute_overlap(b, mask)[0], metrics.compute_alignment(b, mask)[0]


def main():
    _setup()
    import generate_util as gu
    from metrics import metric_layoutnet as metrics
    rs = np.random.RandomState(20231)
    bbox = torch.from_numpy(rs.randn(N_CASES, N_SLOTS, 4)).to(torch.float32).sigmoid()
    num = rs.randint(1, N_SLOTS + 1, size=N_CASES).astype(np.int32)
    mode = (np.arange(N_CASES) % 3).astype(np.uint8)
    jitter = ((np.arange(N_CASES) // 3) % 3 != 2).astype(np.uint8)    # two thirds, every (mode, jitter) combination
    # the factors exactly as the reference forms them (jitter() on a tensor of ones: 1 * f = f), seeds 0..255
    factors = torch.cat([gu.jitter(torch.ones(1, N_SLOTS, 4), s) for s in range(N_CASES)])
    mine = torch.cat([torch.from_numpy(np.random.RandomState(s).uniform(math.log(0.8), math.log(1.2), (1, N_SLOTS, 4))).to(torch.float32).exp() for s in range(N_CASES)])
    assert torch.equal(factors, mine)

    out_b, out_ov, out_al, keep = [], [], [], []
    worst_box = worst_metric = 0.0
    for i in range(N_CASES):
        r32 = run_case(gu, metrics, bbox[i], int(num[i]), bool(jitter[i]), int(mode[i]), i, torch.float32)
        r64 = run_case(gu, metrics, bbox[i], int(num[i]), bool(jitter[i]), int(mode[i]), i, torch.float64)
        db = (r32[0].double() - r64[0]).abs().max().item()
        ok = db <= BOX_TOL
        dm = 0.0
        for a, b in zip(r32[1:], r64[1:]):
            a, b = float(a), float(b)
            ok = ok and math.isfinite(a) and math.isfinite(b) and abs(a - b) <= METRIC_RTOL * abs(b) + METRIC_ATOL
            dm = max(dm, abs(a - b) / (METRIC_RTOL * abs(b) + METRIC_ATOL)) if math.isfinite(a) and math.isfinite(b) else float('inf')
        keep.append(bool(ok))
        if ok:
            worst_box, worst_metric = max(worst_box, db), max(worst_metric, dm)
        out_b.append(r32[0].numpy()); out_ov.append(np.float32(r32[1])); out_al.append(np.float32(r32[2]))
    keep = np.array(keep)
    dropped = int((~keep).sum())
    print(f'dropped {dropped} of {N_CASES} cases (fp32 and fp64 runs of the reference disagree); kept cases agree to {worst_box:.2e} on boxes, '
          f'{worst_metric:.2f} of the metric bar ({METRIC_RTOL:g} relative + {METRIC_ATOL:g})')
    assert dropped <= MAX_DROPPED * N_CASES, f'{dropped} of {N_CASES} cases dropped: more than {MAX_DROPPED:.0%}'
    d = dict(bbox_in=bbox.numpy()[keep], num=num[keep], mode=mode[keep], jitter=jitter[keep], factors=factors.numpy()[keep],
             case_index=np.nonzero(keep)[0].astype(np.int32), bbox_out=np.stack(out_b)[keep], overlap=np.array(out_ov, np.float32)[keep],
             alignment=np.array(out_al, np.float32)[keep], fp64_box_spread=np.float64(worst_box))

    # draws of a few seeds (latents and plan: restated, see the module docstring)
    seeds = [0, 1, 2, 7]
    d['draw_seeds'] = np.array(seeds, np.int64)
    d['latents'] = np.concatenate([torch.from_numpy(np.random.RandomState(s).randn(1, N_SLOTS, 4)).to(torch.float32).numpy() for s in seeds])   # generate_util.py:416, z_dim 4
    d['jitter_factors'] = np.concatenate([gu.jitter(torch.ones(1, N_SLOTS, 4), s).numpy() for s in seeds])
    # draw order of generate_util.py:424-433: per seed a jitter number (none for seed 1: the test on the seed comes first), then an alignment number
    np.random.seed(0)
    plan_seeds = list(range(1, 9))
    pj, pc = [], []
    for seed in plan_seeds:
        pj.append(int(seed != 1 and np.random.rand() < PLAN_PROBS['jitter']))
        pc.append(int(np.random.rand() < PLAN_PROBS['horizontal_center_aligned']))
    d['plan_seeds'] = np.array(plan_seeds, np.int64)
    d['plan_jitter'] = np.array(pj, np.uint8)
    d['plan_center'] = np.array(pc, np.uint8)
    d['plan_probs'] = np.array([PLAN_PROBS['jitter'], PLAN_PROBS['horizontal_center_aligned']])
    np.savez_compressed(OUT, **d)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes;', int(keep.sum()), 'cases')


if __name__ == '__main__':
    main()
