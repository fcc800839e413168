"""Measurements behind the layout-metric kernels (csrc/layoutnet.hip) -> profiles/layout_eval.json.

    python tools/bench_layout_eval.py [--out profiles/layout_eval.json]

Method: warm-up, then a device-synchronised host clock around a block of calls that lasts at least 0.5 s; the two versions of a comparison
alternate in one process (A B A B ...), 7 blocks each; reported: the median, minimum and maximum per-call time over the blocks.
1. LayoutNet.extract_features, N = 9, at B = 8 (the metric loop's batch) and B = 1024: the fused launch against the composed path (the
   generic attention / GEMM / LayerNorm kernels), with the kernel launches per call counted by torch.profiler.
2. FeatureStats.append: ldetr_feature_stats_f64 at n = 8 and n = 1024, F = 256, against the reference's way (copy to the host, float64 GEMM there).
3. One layout-FID generator pass over 2048 synthetic items at batch 8, split into G_ema forward / detector / statistics, and the host Fréchet distance."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))


def block_time(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def alternate(fns, min_block_s=0.5, blocks=7, warmup=20):
    """fns: name -> thunk.  -> name -> dict(median_us, min_us, max_us, calls_per_block)."""
    calls = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        one = block_time(fn, 10)
        calls[name] = max(10, int(min_block_s / max(one, 1e-7)) + 1)
    samples = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            samples[name].append(block_time(fn, calls[name]))
    return {name: dict(median_us=1e6 * float(np.median(v)), min_us=1e6 * min(v), max_us=1e6 * max(v), calls_per_block=calls[name]) for name, v in samples.items()}


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'layout_eval.json'))
    ap.add_argument('--skip-pass', action='store_true')
    args = ap.parse_args()
    import layout_eval_common as C
    from layoutdetr_amd.metrics.layout_frechet_inception_distance import frechet_distance
    from layoutdetr_amd.metrics.metric_utils_layout import FeatureStats
    from layoutdetr_amd.training import networks_layoutnet as nl
    dev = torch.device('cuda:0')
    net = nl.LayoutNet(C.NUM_LABEL)
    net.load_state_dict(C.seeded_layoutnet_state(net))
    net = net.to(dev).eval().requires_grad_(False)
    res = dict(device=torch.cuda.get_device_name(0), method='host clock around >= 0.5 s blocks of calls, device-synchronised; versions alternated; 7 blocks; median [min, max]')

    bbox, label, pad = (t.to(dev) for t in C.seeded_layouts('real'))
    res['extract_features'] = {}
    for B in (8, 1024):
        b, l, p = bbox[:B].contiguous(), label[:B].contiguous(), pad[:B].contiguous()

        def fused():
            with torch.no_grad():
                return net.extract_features(b, l, p)

        def composed():      # the composed path itself, also without autograd (extract_features would pick the fused launch for these arguments)
            with torch.no_grad():
                return net._extract_composed(b, l, p, None)
        n0 = dict(nl.PATH_RUNS); fused(); composed()
        assert nl.PATH_RUNS['fused'] == n0['fused'] + 1 and nl.PATH_RUNS['composed'] == n0['composed'] + 1
        r = alternate(dict(fused=fused, composed=composed))
        r['fused']['launches'] = launches(fused); r['composed']['launches'] = launches(composed)
        r['fused_wins_by_more_than_the_spread'] = bool(r['fused']['max_us'] < r['composed']['min_us'])
        res['extract_features'][f'B{B}'] = r
        print(f'extract_features B={B}:', json.dumps(r), flush=True)

    res['feature_stats'] = {}
    x = torch.randn(1024, 256, device=dev)
    for n in (8, 1024):
        xn = x[:n].contiguous()
        st = FeatureStats(capture_mean_cov=True)
        host = dict(mean=np.zeros(256), cov=np.zeros((256, 256)))

        def device_way():
            st.num_items = 0
            st.append_torch(xn)

        def host_way():
            x64 = xn.cpu().numpy().astype(np.float64)
            host['mean'] += x64.sum(axis=0); host['cov'] += x64.T @ x64
        r = alternate(dict(device_kernel=device_way, host_copy_and_gemm=host_way))
        res['feature_stats'][f'n{n}'] = r
        print(f'feature_stats n={n}:', json.dumps(r), flush=True)

    if not args.skip_pass:
        import bench
        from layoutdetr_amd.training.networks_detr import Generator
        kw = dict(num_bbox_labels=8, img_channels=3, img_height=256, img_width=256, c_dim=0, background_size=256, bert_f_dim=768, bert_num_heads=4,
                  bert_num_encoder_layers=12, bert_num_decoder_layers=2, im_f_dim=512)
        torch.manual_seed(0)
        G = Generator(z_dim=4, f_dim=256, num_heads=4, num_layers=8, text_mode='features', **kw).eval().requires_grad_(False).to(dev)
        net8 = nl.LayoutNet(C.NUM_LABEL)
        net8.load_state_dict(C.seeded_layoutnet_state(net8)); net8 = net8.to(dev).eval().requires_grad_(False)
        bt = bench.to_device_batch(bench.make_batch(8, 256, 'cpu', 3), dev)
        items, B = 2048, 8
        part = dict(G_forward=0.0, detector=0.0, statistics=0.0)
        st = FeatureStats(capture_mean_cov=True, max_items=items)
        with torch.no_grad():
            for it in range(-3, items // B):
                if it == 0:
                    st = FeatureStats(capture_mean_cov=True, max_items=items)
                    part = dict.fromkeys(part, 0.0)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                z = torch.randn([B, 9, G.z_dim], device=dev)
                fake = G(z=z, bbox_class=bt['bbox_class'], bbox_real=bt['bbox_real'], bbox_text=bt['bbox_text'], bbox_patch=bt['bbox_patch'],
                         padding_mask=bt['padding_mask'], background=bt['background'], c=bt['gen_c'])
                torch.cuda.synchronize(); t1 = time.perf_counter()
                f = net8.extract_features(fake, bt['bbox_class'], bt['padding_mask'], label_idx_replace=True)
                torch.cuda.synchronize(); t2 = time.perf_counter()
                st.append_torch(f)
                torch.cuda.synchronize(); t3 = time.perf_counter()
                part['G_forward'] += t1 - t0; part['detector'] += t2 - t1; part['statistics'] += t3 - t2
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for it in range(items // B):      # the same pass without a synchronisation inside: what a metric evaluation runs
                z = torch.randn([B, 9, G.z_dim], device=dev)
                fake = G(z=z, bbox_class=bt['bbox_class'], bbox_real=bt['bbox_real'], bbox_text=bt['bbox_text'], bbox_patch=bt['bbox_patch'],
                         padding_mask=bt['padding_mask'], background=bt['background'], c=bt['gen_c'])
                st.append_torch(net8.extract_features(fake, bt['bbox_class'], bt['padding_mask'], label_idx_replace=True))
            torch.cuda.synchronize(); whole = time.perf_counter() - t0
        mu, sigma = st.get_mean_cov()
        t0 = time.perf_counter(); frechet_distance(mu, sigma, mu + 0.01, sigma * 1.1); t_f = time.perf_counter() - t0
        res['layout_fid_generator_pass'] = dict(items=items, batch=B, background=256, synchronised_parts_s=part, unsynchronised_pass_s=whole, host_frechet_s=t_f,
                                               note='one block each (context, not a comparison); synthetic batch repeated 256 times')
        print('pass:', json.dumps(res['layout_fid_generator_pass']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
