"""Measurements behind LayoutNet.forward and the detector's trainer (csrc/layoutnet_train.hip, layoutdetr_amd/train_layoutnet.py)
-> profiles/layoutnet_train.json.

    python tools/bench_layoutnet_train.py [--out profiles/layoutnet_train.json]                  # the timings
    python tools/bench_layoutnet_train.py --count-launches [--out ...]                           # the launch counts, a run of their own

Method (tools/bench_layout_eval.py's): warm-up, then a device-synchronised host clock around a block of calls that lasts at least 0.5 s; the two
versions of a comparison alternate in one process, 7 blocks each; reported: the median, minimum and maximum per-call time over the blocks.
(a) the evaluation forward (forward_dense, N = 9) at B = 64 and B = 1024: the fused launch against the composed path without autograd;
(b) one training step (LayoutNetTrainer.step: composed forward, loss tail, backward, fused Adam) at batch 64, dropout 0.1.
Kernel launches per call are counted by torch.profiler in the second invocation and merged into the same file."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))
sys.path.insert(2, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'layoutnet_train.json'))
    ap.add_argument('--count-launches', action='store_true')
    args = ap.parse_args()
    import bench_layout_eval as E
    import layout_eval_common as C
    from layoutdetr_amd.train_layoutnet import LayoutNetTrainer
    from layoutdetr_amd.training import networks_layoutnet as nl
    dev = torch.device('cuda:0')

    def network():
        net = nl.LayoutNet(C.NUM_LABEL)
        net.load_state_dict(C.seeded_layoutnet_state(net))
        return net.to(dev).eval().requires_grad_(False)
    net = network()
    res = json.load(open(args.out)) if (args.count_launches and os.path.exists(args.out)) else {}
    res.update(device=torch.cuda.get_device_name(0), method='host clock around >= 0.5 s blocks of calls, device-synchronised; versions alternated; 7 blocks; '
               'median [min, max]; launches: torch.profiler, in a process of its own')
    bbox, label, pad = (t.to(dev) for t in C.seeded_layouts('real'))
    res.setdefault('forward_eval', {})
    for B in (64, 1024):
        b, l, p = bbox[:B].contiguous(), label[:B].contiguous(), pad[:B].contiguous()

        def fused():
            with torch.no_grad():
                return net.forward_dense(b, l, p)

        def composed():      # the composed path itself, also without autograd (forward_dense would pick the fused launch for these arguments)
            with torch.no_grad():
                return net._forward_composed(b, l, p)
        n0 = dict(nl.PATH_RUNS); fused(); composed()
        assert nl.PATH_RUNS['forward_fused'] == n0['forward_fused'] + 1 and nl.PATH_RUNS['forward_composed'] == n0['forward_composed'] + 1
        r = res['forward_eval'].setdefault(f'B{B}', dict(fused={}, composed={}))
        if args.count_launches:
            r['fused']['launches'] = E.launches(fused); r['composed']['launches'] = E.launches(composed)
        else:
            t = E.alternate(dict(fused=fused, composed=composed))
            r['fused'].update(t['fused']); r['composed'].update(t['composed'])
            r['fused_wins_by_more_than_the_spread'] = bool(r['fused']['max_us'] < r['composed']['min_us'])
        print(f'forward_eval B={B}:', json.dumps(r), flush=True)

    tnet = network()
    trainer = LayoutNetTrainer(tnet, lr=1e-4, dropout=0.1)
    b, l, p = bbox[:64].contiguous(), label[:64].contiguous(), pad[:64].contiguous()
    real = torch.arange(64, device=dev) % 2 == 0

    def step():
        return trainer.step(b, l, p, real)
    r = res.setdefault('train_step_B64', {})
    if args.count_launches:
        r['launches'] = E.launches(step)
    else:
        r.update(E.alternate(dict(step=step))['step'])
    print('train_step_B64:', json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
