#!/usr/bin/env python
"""Stand-alone timing of the encoder rider: two 6-layer 64-token encoders (d 256, 8 heads, feed-forward 2048, dropout on) forward, one after the other
against lock-step (TransformerEncoder.forward(rider=)), at the row counts of the two main phases at 16 samples (1024 + 1024, 2048 + 1024) and at 2
(128 + 128, 256 + 128).  Each variant is captured in a graph and the graph replayed; device events around the replays, five windows, sorted.

    python tools/bench_enc_rider.py      -> one line per case, then all of them as one JSON line ([fastest .. slowest] window, us per pair of forwards)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdetr_amd.hip import core, rider  # noqa: E402
from layoutdetr_amd.training.detr_transformer import TransformerEncoder, TransformerEncoderLayer  # noqa: E402

dev = torch.device('cuda:0')


def timed(fn, replays=20):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    best = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        best.append(round(e0.elapsed_time(e1) * 1000.0 / replays, 1))
    return sorted(best)


torch.manual_seed(0)
core.lib()
encs = [TransformerEncoder(TransformerEncoderLayer(256, 8, 2048, 0.1), 6).to(dev).train().requires_grad_(False) for _ in range(2)]
out = {}
for ba, bb in ((16, 16), (32, 16), (2, 2), (4, 2)):
    xs = [torch.randn(b * 64, 256, device=dev) for b in (ba, bb)]
    ps = [torch.randn(b * 64, 256, device=dev) for b in (ba, bb)]
    ks = [torch.zeros(b, 64, dtype=torch.bool, device=dev) for b in (ba, bb)]

    def apart():
        with torch.no_grad():
            for e, x, p, k, b in zip(encs, xs, ps, ks, (ba, bb)):
                e.forward2d(x, b, 64, k, p, want_pos=True)

    def lockstep():
        with torch.no_grad():
            encs[0](xs[0], ba, 64, ks[0], ps[0], want_pos=True, rider=(encs[1], xs[1], bb, 64, ks[1], ps[1]))
    before = dict(rider.STATS)
    a, l = timed(apart), timed(lockstep)
    sent = {k: rider.STATS[k] - before[k] for k in before}
    out[f'rows {ba * 64} + {bb * 64}'] = dict(apart_us=[a[0], a[-1]], lockstep_us=[l[0], l[-1]], ratio=round(l[2] / a[2], 3), launches_per_capture={k: v // 2 for k, v in sent.items()})
    print(f'rows {ba * 64} + {bb * 64}: apart {a[0]} .. {a[-1]} us, lock-step {l[0]} .. {l[-1]} us, ratio {l[2] / a[2]:.3f}, {sent}', flush=True)
print(json.dumps(out))
