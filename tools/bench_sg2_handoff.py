"""Time and algorithmic bandwidth of the synthesis backward's hand-off kernel (ldetr_sg2_handoff_f32) next to the launches it replaces
(toRGB backward, autograd's add of the two dx, `* styles` + style sum, lrelu backward + bias / demodulation sums), same process, same shapes.
Algorithmic bytes = the tensors a launch must read or write at least once."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from layoutdetr_amd.hip import core
dev = torch.device('cuda:0')
def timeit(fn, n=10):
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n): fn()
    g.replay(); torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record(); g.replay(); e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e-3
L = core.lib(); p = core.ptr
for (B, R, C, modes) in [(16, 256, 32, ('conv+rgb', 'conv', 'rgb')), (16, 128, 64, ('conv+rgb',)), (16, 64, 128, ('conv+rgb',))]:
    P = R * R
    dxs = torch.randn(B, P, C, device=dev); x = torch.randn(B, P, C, device=dev); dy = torch.randn(B, P, 3, device=dev)
    sc = torch.rand(B, C, device=dev) + 0.5; sr = torch.rand(B, C, device=dev) + 0.5; w = torch.randn(3, C, device=dev)
    bias = torch.randn(C, device=dev); demod = torch.rand(B, C, device=dev) + 0.5
    ds = torch.zeros(B, C, device=dev); dws = torch.zeros(B, 3, C, device=dev); dbr = torch.zeros(3, device=dev); db = torch.zeros(C, device=dev); dd = torch.zeros(B, C, device=dev)
    dx_rgb = torch.empty_like(x); dsum = torch.empty_like(x); dxo = torch.empty_like(x); dv = torch.empty_like(x)
    T = x.numel() * 4
    for mode in modes:
        conv, rgb = 'conv' in mode, 'rgb' in mode
        def new():
            L.ldetr_sg2_handoff_f32(p(dxs) if conv else None, p(x), p(dy) if rgb else None, p(dv), p(sc) if conv else None, p(sr) if rgb else None, p(w) if rgb else None,
                                    p(bias), p(demod), p(ds) if conv else None, p(dws) if rgb else None, p(dbr) if rgb else None, p(db), p(dd), B, P, C, 0.2, 1.414, core.stream())
        def old():
            g = dxs
            if conv:
                L.ldetr_mul_reduce_f32(p(dxs), p(x), p(sc), p(dxo), p(ds), B, P, C, core.stream()); g = dxo
            if rgb:
                L.ldetr_torgb_bwd_f32(p(x), p(dy), p(w), p(sr), p(dx_rgb), p(dws), p(dbr), B, P, C, core.stream()); g = dx_rgb
            if conv and rgb:
                torch.add(dxo, dx_rgb, out=dsum); g = dsum
            L.ldetr_act_bwd_reduce_f32(p(g), p(x), p(dv), p(bias), p(demod), p(db), p(dd), B, P, C, 2, 0.2, 1.414, core.stream())
        tn, to = timeit(new), timeit(old)
        nb = T * ((2 if conv else 1) + 1) + (dy.numel() * 4 if rgb else 0)                      # new: read dxs?, x, dy?; write dv
        ob = T * ((3 if conv else 0) + (2 if rgb else 0) + (3 if conv and rgb else 0) + 3) + (dy.numel() * 4 if rgb else 0)
        print(f'B={B:2d} {R:3d}^2 C={C:3d} {mode:8s}: hand-off {tn*1e6:7.1f} us {nb/1e6:6.1f} MB {nb/tn/1e12:5.2f} TB/s | replaced launches {to*1e6:7.1f} us {ob/1e6:7.1f} MB '
              f'{ob/to/1e12:5.2f} TB/s | {to/tn:4.2f}x', flush=True)
