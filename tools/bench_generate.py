"""Measurements behind layout generation (layoutdetr_amd/generate.py) -> profiles/generate_bench.json, one JSON line on stdout.

    python tools/bench_generate.py [--out profiles/generate_bench.json]

C = 1 condition, K in {1, 4, 16, 64} candidates, backgrounds 256 x 256 and 1024 x 1024, TextFeatures in (the text encoder is a boundary input).
  (a) reference_pattern   K separate G(...) eval calls with batch 1 (generate_util.py:415-423): runs identically on the parent commit -- the baseline
  (b) encode_sample       Sampler.encode + Sampler.sample (centre-aligned, jittered)
  (c) sample              Sampler.sample alone on a held Condition ("the same banner, more variations")
  (d) finish              the finishing launch alone on K layouts
Method: warm-up, then blocks of calls that last at least 0.2 s (at least 3 calls), each block timed twice over: by a pair of device events
recorded around it on the stream (`*_us`: the span the device saw) and by a host clock between two synchronisations (`host_*_us`).  The four
versions alternate in one process (a b c d a b c d ...), 5 blocks each; reported: the median, minimum and maximum per-call time over the
blocks.  Every version is bound by launches, not by arithmetic, so the two clocks agree to the cost of one synchronisation per block; what a
caller waits for is the host figure.  `decoder_share_of_sample` is the median over 5 alternated pairs of blocks of decode_candidates alone over
sample.  Kernel launches per call are counted by torch.profiler."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def block_time(fn, calls):
    """-> (device seconds per call between two events, host seconds per call between two synchronisations)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls, (time.perf_counter() - t0) / calls


def _stats(v, prefix=''):
    return {prefix + 'median_us': 1e6 * float(np.median(v)), prefix + 'min_us': 1e6 * min(v), prefix + 'max_us': 1e6 * max(v)}


def alternate(fns, min_block_s=0.2, blocks=5, warmup=3, min_calls=3):
    calls = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        one = block_time(fn, min_calls)[1]
        calls[name] = max(min_calls, int(min_block_s / max(one, 1e-7)) + 1)
    samples = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            samples[name].append(block_time(fn, calls[name]))
    return {name: dict(_stats([d for d, _ in v]), **_stats([h for _, h in v], 'host_'), calls_per_block=calls[name]) for name, v in samples.items()}


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
    except Exception as e:       # a profiler that is not available must not cost the timings
        return f'not counted ({type(e).__name__})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'generate_bench.json'))
    ap.add_argument('--sizes', default='256,1024')
    ap.add_argument('--ks', default='1,4,16,64')
    args = ap.parse_args()
    from layoutdetr_amd.generate import CENTER, Sampler, jitter_factors, layout_finish
    from layoutdetr_amd.training.networks_detr import Generator, TextFeatures
    dev = torch.device('cuda:0')
    from layoutdetr_amd.training import shared_decode
    res = dict(device=torch.cuda.get_device_name(0), conditions=1, candidates_per_decoder_pass=shared_decode.CHUNK,
               method='device events (and, host_*, a synchronised host clock) around >= 0.2 s blocks of calls (>= 3); versions alternated; 5 blocks; '
                      'median [min, max] in us per call',
               cases={})
    g = torch.Generator().manual_seed(0)
    n_valid = 4
    cls = torch.randint(0, 8, (1, 9), generator=g).to(dev)
    tf = TextFeatures(torch.randn(1, 9, 768, generator=g).to(dev), torch.randint(1, 40, (1, 9), generator=g).to(dev))
    pm = (torch.arange(9)[None, :] >= n_valid).to(dev)
    patch = torch.zeros(1, 9, 1, 1, 1, device=dev)
    for S in [int(v) for v in args.sizes.split(',')]:
        torch.manual_seed(0)
        G = Generator(z_dim=4, num_bbox_labels=8, img_channels=3, img_height=S, img_width=S, c_dim=0, background_size=S, bert_f_dim=768, im_f_dim=512,
                      text_mode='features').eval().requires_grad_(False).to(dev)
        smp = Sampler(G)
        bgd = torch.randn(1, 3, S, S, generator=g).to(dev)
        for K in [int(v) for v in args.ks.split(',')]:
            seeds = list(range(1, K + 1))
            zs = [torch.randn(1, 9, 4, generator=g).to(dev) for _ in range(K)]
            plan = dict(jitter=[True] * K, modes=[CENTER] * K)
            held = smp.encode(bgd, tf, cls, padding_mask=pm)
            boxes = torch.rand(1, K, 9, 4, generator=g).to(dev)
            num = torch.full((1, K), n_valid, dtype=torch.int32, device=dev)
            fac = jitter_factors(seeds).to(dev).unsqueeze(0)
            flags = torch.ones(1, K, dtype=torch.uint8, device=dev)

            def reference_pattern():
                with torch.no_grad():
                    return [G(z, cls, None, tf, patch, pm, bgd, None) for z in zs]

            def encode_sample():
                return smp.sample(smp.encode(bgd, tf, cls, padding_mask=pm), seeds=seeds, **plan)

            def sample():
                return smp.sample(held, seeds=seeds, **plan)

            def finish():
                return layout_finish(boxes, num, fac, flags, flags)
            r = alternate(dict(reference_pattern=reference_pattern, encode_sample=encode_sample, sample=sample, finish=finish))
            r['encode_sample']['launches'] = launches(encode_sample)
            r['sample']['launches'] = launches(sample)
            r['reference_pattern']['launches'] = launches(reference_pattern)

            def decode_only():
                return G.decode_candidates(held, torch.cat(zs))
            r['decoder_share_of_sample'] = float(np.median([block_time(decode_only, 10)[0] / block_time(sample, 10)[0] for _ in range(5)]))
            r['encode_sample_beats_reference_pattern_by_more_than_the_spread'] = bool(r['encode_sample']['max_us'] < r['reference_pattern']['min_us'])
            res['cases'][f'bg{S}_K{K}'] = r
            print(f'bg {S} K {K}:', json.dumps(r), file=sys.stderr, flush=True)
        del G, smp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
