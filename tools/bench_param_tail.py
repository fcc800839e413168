#!/usr/bin/env python
"""Stand-alone timings of the per-step parameter tail: the LayerNorm backward at the token stacks' row counts (next to the forward at the same rows),
the fused Adam step at beta1 = 0 at D's and G's parameter counts, and one ldetr_p3_weight_prep launch over a ResNet-50 trunk's weights.  Each kernel
is captured 4-50 times in a graph and the graph replayed; device events around the replays, five windows, sorted.

    python tools/bench_param_tail.py <tag> [lnonly]      -> one line per case, then all of them as one JSON line ([fastest .. slowest] window, us)

One process per build (LDETR_LIB=<the parent commit's library>) or knob setting (LDETR_DEBUG=LN_BWD_WIDE_ROWS=...)."""
import os
import sys
import json
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdetr_amd.hip import blocks, core  # noqa: E402

dev = torch.device('cuda:0')
tag = sys.argv[1]
out = {}


def timed(fn, reps_in_graph, replays=20):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(reps_in_graph):
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
        best.append(e0.elapsed_time(e1) * 1000.0 / (replays * reps_in_graph))
    return sorted(best)


L = core.lib()
# ---- LayerNorm backward, D = 256, one problem; ln_fwd at the same rows for scale
for rows in (144, 192, 256, 320, 1024, 2048):
    D = 256
    x = torch.randn(rows, D, device=dev); dy = torch.randn(rows, D, device=dev); gamma = torch.rand(D, device=dev) + 0.5; beta = torch.randn(D, device=dev)
    y = torch.empty_like(x); z = torch.empty_like(x); mean = torch.empty(rows, device=dev); rstd = torch.empty(rows, device=dev)
    r = torch.randn(rows, D, device=dev)
    dx = torch.empty_like(x); dr = torch.empty_like(x); dg = torch.zeros(D, device=dev); db = torch.zeros(D, device=dev)
    af = blocks.ln_fwd(x, r, gamma, beta, 1e-5, 0.1, 5, y, z, mean, rstd)
    blocks.launch('layernorm_fwd', [af])
    ab = blocks.ln_bwd(dy, z, mean, rstd, gamma, dx, dr, dg, db, 0.1, 5)
    t = timed(lambda: blocks.launch('layernorm_bwd', [ab]), 50)
    tf = timed(lambda: blocks.launch('layernorm_fwd', [af]), 50)
    out[f'ln_bwd rows {rows}'] = t
    out[f'ln_fwd rows {rows}'] = tf
    print(f'[{tag}] ln_bwd rows {rows}: {t[0]:.2f} .. {t[-1]:.2f} us   (ln_fwd {tf[0]:.2f} .. {tf[-1]:.2f})', flush=True)

if len(sys.argv) > 2 and sys.argv[2] == 'lnonly':
    print(json.dumps({tag: out}))
    sys.exit(0)
# ---- Adam at beta1 = 0: D's and G's sizes
for n, ema in ((90_000_000, False), (45_000_000, True)):
    p = torch.randn(n, device=dev); g = torch.randn(n, device=dev); m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev)
    pe = torch.randn(n, device=dev) if ema else None

    def step():
        args = (core.ptr(p), core.ptr(g), core.ptr(m), core.ptr(v), n, 5, 0.002, 0.0, 0.99, 1e-8, 1, 0.5, 0.0, 1e5, -1e5)
        if ema:
            core.check(L.ldetr_adam_ema_step_f32(*args, core.ptr(pe), 0.999, core.stream()), 'adam')
        else:
            core.check(L.ldetr_adam_step_f32(*args, core.stream()), 'adam')
    t = timed(step, 4, replays=5)
    out[f'adam n {n} ema {int(ema)}'] = t
    print(f'[{tag}] adam n {n} ema {int(ema)}: {t[0]:.1f} .. {t[-1]:.1f} us', flush=True)
    del p, g, m, v, pe

# ---- weight images of a ResNet-50 trunk (the P3 convs: everything but the stem)
shapes = []
inpl = 64
for planes, nblk in ((64, 3), (128, 4), (256, 6), (512, 3)):
    for b in range(nblk):
        shapes += [(planes, inpl, 1), (planes, planes, 9), (planes * 4, planes, 1)]
        if b == 0:
            shapes.append((planes * 4, inpl, 1))
        inpl = planes * 4
ws = [torch.randn(O, T, 1, I, device=dev) * 0.05 for O, I, T in shapes]
scs = [torch.rand(O, device=dev) + 0.5 for O, I, T in shapes]
total = sum(w.numel() * 6 for w in ws)
fwd = torch.empty(total, dtype=torch.uint8, device=dev); bwd = torch.empty(total, dtype=torch.uint8, device=dev)
rows_, off, blk = [], 0, 0
for w, sc in zip(ws, scs):
    O, T, _, I = w.shape
    rows_.append([w.data_ptr(), sc.data_ptr(), fwd.data_ptr() + off, bwd.data_ptr() + off, O, T, I, blk])
    off += w.numel() * 6; blk += (w.numel() // 8 + 255) // 256
tab = torch.tensor(rows_, dtype=torch.int64, device=dev)
t = timed(lambda: core.check(L.ldetr_p3_weight_prep(core.ptr(tab), len(ws), blk, core.stream()), 'prep'), 4, replays=5)
out['weight_prep resnet50'] = t
print(f'[{tag}] weight_prep {sum(w.numel() for w in ws) / 1e6:.1f} M weights: {t[0]:.1f} .. {t[-1]:.1f} us', flush=True)
print(json.dumps({tag: out}))
