"""The StyleGAN2 synthesis network (training/networks_stylegan2.py SynthesisNetwork, architecture 'skip') as ONE autograd node.

Forward: the launches of the per-layer Functions (hip/modconv.py) in their order.  What the node buys is the backward: between two
contraction launches the per-layer graph runs toRGB's backward (a full dx), autograd's sum of the two dx, the consumer conv's `* styles`
pass with its style sum and the producer's lrelu backward with its bias / demodulation sums -- four passes over the same two tensors.
Here they are one streaming launch per layer boundary (ldetr_sg2_handoff_f32, csrc/misc_ops.hip): the producer's saved output is at once
the tensor the style gradient multiplies against, the toRGB's input and the carrier of the lrelu sign.  The up layer's <dud, ud> / d
comes out of the same launch as <dv, pre(y) - bias> / d (4 FIR(ud) = pre(y) - bias, dud = 4 FIR^T(dv)), so `ud` is not saved.

The affines and the demodulation coefficients stay ordinary autograd nodes in front of this one (SynthesisNetwork.forward)."""
import torch

from . import core, modconv
from .conv import weight_ohwi
from ..torch_utils.ops import upfirdn2d as _up

ENABLED = core.knob('SG2_CHAIN', 1) != 0     # 0: every layer as its own autograd node (A/B and equivalence tests)
ACT_ALPHA = 0.2
NODE_RUNS = [0]


class Block(object):
    """One resolution of the network for the node: which layers it has and the Parameters behind them (for the flat gradient views)."""

    def __init__(self, has_conv0, gains, params):
        self.has_conv0 = has_conv0
        self.gains = gains           # activation gains of (conv0, conv1); conv0's is None at the first block
        self.params = params         # dict: 'conv0' / 'conv1' / 'torgb' -> (weight Parameter, bias Parameter)


def _handoff(dxs, x, dy_rgb, s_conv, rgb, bias, demod, dbias, gain):
    """-> dv (in dxs's memory when there is one), ds_conv, dws_rgb, ddemod.  rgb = (s_rgb, w_rgb [3, C], dbias_rgb) or None."""
    B, H, W, C = x.shape
    dev = x.device
    dv = dxs if dxs is not None else torch.empty_like(x)
    ds_conv = core.zeros((B, C), dev) if dxs is not None else None
    dws = core.zeros((B, 3, C), dev) if dy_rgb is not None else None
    ddemod = core.zeros((B, C), dev)
    s_rgb, w_rgb, dbias_rgb = rgb if dy_rgb is not None else (None, None, None)
    core.check(core.lib().ldetr_sg2_handoff_f32(core.ptr(dxs), core.ptr(x), core.ptr(dy_rgb), core.ptr(dv), core.ptr(s_conv), core.ptr(s_rgb), core.ptr(w_rgb),
                                                core.ptr(bias), core.ptr(demod), core.ptr(ds_conv), core.ptr(dws), core.ptr(dbias_rgb), core.ptr(dbias),
                                                core.ptr(ddemod), B, H * W, C, ACT_ALPHA, gain, core.stream()), 'sg2_handoff')
    return dv, ds_conv, dws, ddemod


def _bias_target(bparam, C, device):
    """-> (buffer the bias gradient is accumulated into, it is the flat .grad view)."""
    gb = core.flat_grad(bparam)
    if gb is not None:
        return gb, True
    return torch.zeros(C, device=device, dtype=torch.float32), False       # (returned to autograd as a parameter gradient: never arena memory)


class _SynthesisFn(torch.autograd.Function):
    """forward(blocks, const, f, *tensors) -> image NHWC [B, R, R, 3].  tensors, per block from 4x4 up:
    [conv0: weight, bias, styles, dcoefs]  conv1: weight, bias, styles, dcoefs  torgb: weight, bias, styles (weight gain included)."""

    @staticmethod
    def forward(ctx, blocks, const, f, *tensors):
        core.require_gpu(const, f, *tensors)
        keep = any(ctx.needs_input_grad)         # under no_grad (G_ema, generation) nothing is kept
        it = iter(tensors)
        saved, layout = [const, f], []
        x = img = None
        B = tensors[2].shape[0]
        for blk in blocks:
            entry = {}
            if blk.has_conv0:
                w, b, s, d = [next(it) for _ in range(4)]
                w = core.f32c(weight_ohwi(w)); b = core.f32c(b); s = core.f32c(s); d = core.f32c(d)
                _, x0 = modconv.up_fwd(x, w, s, d, b, f, ACT_ALPHA, blk.gains[0])
                entry['conv0'] = (w, b, s, d, x0)
                x = x0
            else:
                x = core.f32c(const).permute(1, 2, 0).unsqueeze(0).repeat([B, 1, 1, 1])
                entry['xin'] = (x,)
            w, b, s, d = [next(it) for _ in range(4)]
            w = core.f32c(weight_ohwi(w)); b = core.f32c(b); s = core.f32c(s); d = core.f32c(d)
            x = modconv.conv_fwd(x, w, s, d, b, w.shape[1] // 2, ACT_ALPHA, blk.gains[1])
            entry['conv1'] = (w, b, s, d, x)
            if img is not None:
                # upfirdn2d.upsample2d with the 4-tap filter: up 2, pad [2, 1, 2, 1], gain 4
                img = _up._kernel_call(img.permute(0, 3, 1, 2), f, 2, 2, 1, 1, 2, 1, 2, 1, False, 4.0).permute(0, 2, 3, 1)
            w, b, s = [next(it) for _ in range(3)]
            ctx_wshape = w.shape
            w = core.f32c(w.reshape(w.shape[0], -1)); b = core.f32c(b); s = core.f32c(s)
            if w.shape[0] != 3:
                raise NotImplementedError('the synthesis node is specialised for 3 colour channels')
            y = modconv.torgb_fwd(x, w, s, b)
            img = img + y if img is not None else y
            entry['torgb'] = (w, s)
            entry['rgb_wshape'] = ctx_wshape
            if keep:
                rec = {}
                for k in ('conv0', 'xin', 'conv1', 'torgb'):
                    if k in entry:
                        rec[k] = (len(saved), len(entry[k]))
                        saved += list(entry[k])
                rec['rgb_wshape'] = ctx_wshape
                layout.append(rec)
        if keep:
            ctx.save_for_backward(*saved)
            ctx.blocks, ctx.layout = blocks, layout
        return img

    @staticmethod
    def backward(ctx, dimg):
        saved = ctx.saved_tensors
        const, f = saved[0], saved[1]
        blocks, layout = ctx.blocks, ctx.layout
        need = ctx.needs_input_grad[3:]
        get = lambda rec, k: saved[rec[k][0]:rec[k][0] + rec[k][1]]
        dimg = core.f32c(dimg)
        dev = dimg.device
        grads = [None] * len(need)
        # position of each block's first tensor in `tensors`
        first, n = [], 0
        for blk in blocks:
            first.append(n)
            n += 11 if blk.has_conv0 else 7
        dxs_next = s_next = dconst = None       # the conv above's data gradient (before its styles) and that conv's styles
        for i in reversed(range(len(blocks))):
            blk, rec = blocks[i], layout[i]
            o = first[i] + (4 if blk.has_conv0 else 0)          # conv1's weight; the toRGB's is at o + 4
            w1, b1, s1, d1, x1 = get(rec, 'conv1')
            wr, sr = get(rec, 'torgb')
            B, H, W, C = x1.shape
            (w1p, b1p), (wrp, brp) = blk.params['conv1'], blk.params['torgb']
            # hand-off into conv1: toRGB's and the next block's conv0's gradients meet at conv1's output
            dw_rgb, dbias_rgb, wr_flat, br_flat = modconv.torgb_grad_targets(wrp, brp, 3, C, dev)
            db1, b1_flat = _bias_target(b1p, C, dev)
            dv1, ds_next, dws, dd1 = _handoff(dxs_next, x1, dimg, s_next, (sr, wr, dbias_rgb), b1, d1, db1, blk.gains[1])
            ds_rgb = torch.empty((B, C), device=dev, dtype=torch.float32)
            core.check(core.lib().ldetr_torgb_bwd_finish_f32(core.ptr(dws), core.ptr(sr), core.ptr(wr), B, C, core.ptr(dw_rgb), core.ptr(ds_rgb), core.stream()),
                       'torgb_bwd_finish')
            if i + 1 < len(blocks):
                grads[first[i + 1] + 2] = ds_next
            grads[o + 4] = None if wr_flat else dw_rgb.reshape(rec['rgb_wshape'])
            grads[o + 5] = None if br_flat else dbias_rgb
            grads[o + 6] = ds_rgb
            grads[o + 1] = None if b1_flat else db1
            grads[o + 3] = dd1
            # conv1
            xin = get(rec, 'conv0')[4] if blk.has_conv0 else get(rec, 'xin')[0]
            pad = w1.shape[1] // 2
            dxs1 = modconv.conv_bwd_data(dv1, w1, d1, B, xin.shape[1], xin.shape[2], pad)
            if need[o]:
                grads[o] = modconv.conv_bwd_weight(xin, dv1, w1, s1, d1, w1p, pad)
            if not blk.has_conv0:
                # the 4x4 block: its input is the constant, expanded over the batch
                dx, ds1 = modconv._mul_reduce(dxs1, xin, s1, B, xin.shape[1] * xin.shape[2], xin.shape[3])
                grads[o + 2] = ds1
                if ctx.needs_input_grad[1]:
                    dconst = dx.sum(0).permute(2, 0, 1)
                break
            # hand-off conv1 -> conv0, FIR adjoint, transposed conv
            w0, b0, s0, d0, x0 = get(rec, 'conv0')
            w0p, b0p = blk.params['conv0']
            db0, b0_flat = _bias_target(b0p, C, dev)
            dv0, ds1, _, dd0 = _handoff(dxs1, x0, None, s1, None, b0, d0, db0, blk.gains[0])
            grads[o + 2] = ds1
            grads[first[i] + 1] = None if b0_flat else db0
            grads[first[i] + 3] = dd0
            dud = modconv.up_fir_adjoint(dv0, f)
            xprev = get(layout[i - 1], 'conv1')[4]
            dxs_next = modconv.up_bwd_data(dud, w0, d0, B, xprev.shape[1], xprev.shape[2])
            s_next = s0
            if need[first[i]]:
                grads[first[i]] = modconv.up_bwd_weight(xprev, dud, w0, s0, d0, w0p)
            # adjoint of upsample2d on the 3-channel image gradient: down 2, pad [1, 1, 1, 1], flipped taps, gain 4
            dimg = _up._kernel_call(dimg.permute(0, 3, 1, 2), f, 1, 1, 2, 2, 1, 1, 1, 1, True, 4.0).permute(0, 2, 3, 1)
        return (None, dconst, None) + tuple(grads)


def run(blocks, const, f, tensors):
    """-> image NHWC [B, R, R, 3]."""
    NODE_RUNS[0] += 1
    return _SynthesisFn.apply(blocks, const, f, *tensors)
