"""The StyleGAN2 synthesis network (training/networks_stylegan2.py SynthesisNetwork, architecture 'skip') as ONE autograd node.

Forward: the launches of the per-layer Functions (hip/modconv.py) in their order.  What the node buys is the backward: between two
contraction launches the per-layer graph runs toRGB's backward (a full dx), autograd's sum of the two dx, the consumer conv's `* styles`
pass with its style sum and the producer's lrelu backward with its bias / demodulation sums -- four passes over the same two tensors.
Here they are one streaming launch per layer boundary (ldetr_sg2_handoff_f32, csrc/misc_ops.hip): the producer's saved output is at once
the tensor the style gradient multiplies against, the toRGB's input and the carrier of the lrelu sign.  The up layer's <dud, ud> / d
comes out of the same launch as <dv, pre(y) - bias> / d (4 FIR(ud) = pre(y) - bias, dud = 4 FIR^T(dv)), so `ud` is not saved.

The side chain -- the per-layer style affines and demodulation coefficients -- belongs to the node too when one latent [B, w_dim] feeds
every layer (what the Decoder's mapping network produces): all styles are ONE grouped small-GEMM launch (core.gemm_group, the toRGB
weight gain as its post factor), all coefficient sets ONE grouped demodulation launch, and the backward ends with one grouped demodulation
backward (its style part adds into the style gradients the hand-offs produced) and the affine backward over all layers
(ldetr_sg2_affine_bwd_f32: the latent's gradient as one product over the concatenated channels).  The toRGB launches add the upsampled
image of the block below themselves.  LDETR_DEBUG="SG2_SIDE=0", per-layer latents, more than 64 samples and affines of another form keep
the side chain as ordinary autograd nodes in front of the node (SynthesisNetwork._forward_node)."""

import torch

from . import core, modconv
from .. import _lib
from .conv import weight_ohwi
from ..torch_utils.ops import upfirdn2d as _up

ENABLED = core.knob('SG2_CHAIN', 1) != 0     # 0: every layer as its own autograd node (A/B and equivalence tests)
SIDE = core.knob('SG2_SIDE', 1) != 0         # 0: affines and demodulation coefficients as autograd nodes in front of the node
ACT_ALPHA = 0.2
NODE_RUNS = [0]
SIDE_MAX_B = 64                              # the grouped demodulation / affine kernels keep one value per sample in LDS
DEMOD_GROUP_MAX, AFFINE_GROUP_MAX = 24, 32   # LDETR_DEMOD_GROUP_MAX, LDETR_AFFINE_GROUP_MAX


class Block(object):
    """One resolution of the network for the node: which layers it has and the Parameters behind them (for the flat gradient views)."""

    def __init__(self, has_conv0, gains, params, affines=None):
        self.has_conv0 = has_conv0
        self.gains = gains           # activation gains of (conv0, conv1); conv0's is None at the first block
        self.params = params         # dict: 'conv0' / 'conv1' / 'torgb' -> (weight Parameter, bias Parameter)
        self.affines = affines       # side chain inside the node: same keys -> (affine weight Parameter, affine bias Parameter, weight gain, post factor)


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


def _views(flat, shapes):
    """Consecutive views of `flat`, one per shape (every size a multiple of 4 floats keeps them 16-byte aligned)."""
    out, o = [], 0
    for shp in shapes:
        n = shp[0] * shp[1]
        out.append(flat[o:o + n].view(shp))
        o += n
    return out


def side_styles(ws, affines):
    """affines: (weight [C, D], bias [C], weight gain, post factor) per layer -> styles [B, C] per layer, the grouped form of
    FullyConnectedLayer.forward (`linear(w, weight, bias, wscale=gain)`, then `* post` for a toRGB): bit-equal to it."""
    B, D = ws.shape
    dev = ws.device
    shapes = [(B, a[0].shape[0]) for a in affines]
    styles = _views(torch.empty(sum(b * c for b, c in shapes), device=dev, dtype=torch.float32), shapes)
    problems = [dict(A=ws, B=a[0], M=B, N=a[0].shape[0], K=D, out=s, ep=core.epilogue(alpha=a[2], col_bias=a[1])) for a, s in zip(affines, styles)]
    posts = [a[3] for a in affines]
    for i in range(0, len(problems), core.GEMM_GROUP_MAX):
        chunk, post = problems[i:i + core.GEMM_GROUP_MAX], posts[i:i + core.GEMM_GROUP_MAX]
        if not core.gemm_group(chunk, post):
            for g, ps in zip(chunk, post):       # (a group the library does not run as one launch: the same problems one by one)
                core.gemm(g['A'], g['B'], 0, 0, g['M'], g['N'], g['K'], out=g['out'], ep=g['ep'])
                if ps != 1.0:
                    g['out'].mul_(ps)
    return styles


def _demod_descs(layers, grads=None):
    """layers: (weight [O, I, KH, KW] any strides, styles, dcoefs, w2) -> ldetr_demod_desc array; grads: (grad_dcoefs, dweight or None, dstyles) per layer."""
    descs = (_lib.DemodDesc * len(layers))()
    for i, (d, (w, s, dc, w2)) in enumerate(zip(descs, layers)):
        d.weight = w.data_ptr()
        d.so, d.si, d.sh, d.sw = w.stride()
        d.styles, d.dcoefs, d.w2 = s.data_ptr(), dc.data_ptr(), w2.data_ptr()
        d.O, d.I, d.KH, d.KW = w.shape
        if grads is not None:
            g, dw, ds = grads[i]
            d.grad_dcoefs, d.dweight, d.dstyles = g.data_ptr(), (dw.data_ptr() if dw is not None else None), ds.data_ptr()
    return descs


def side_demod(weights, styles):
    """Demodulation coefficients of every layer as one launch (ldetr_demod_group_fwd_f32; bit-equal to modconv.demod_coefs per layer).
    weights: fp32 [O, I, KH, KW] tensors (any strides) -> (dcoefs [B, O] per layer, w2 [O, I] per layer)."""
    B = styles[0].shape[0]
    dev = styles[0].device
    dshapes = [(B, w.shape[0]) for w in weights]
    wshapes = [(w.shape[0], w.shape[1]) for w in weights]
    dcoefs = _views(torch.empty(sum(a * b for a, b in dshapes), device=dev, dtype=torch.float32), dshapes)
    w2 = _views(torch.empty(sum(a * b for a, b in wshapes), device=dev, dtype=torch.float32), wshapes)
    layers = list(zip(weights, styles, dcoefs, w2))
    for i in range(0, len(layers), DEMOD_GROUP_MAX):
        chunk = layers[i:i + DEMOD_GROUP_MAX]
        core.check(core.lib().ldetr_demod_group_fwd_f32(_demod_descs(chunk), len(chunk), B, 1e-8, core.stream()), 'demod_group_fwd')
    return dcoefs, w2


def side_demod_bwd(layers, grads, B):
    """layers as _demod_descs; grads: (grad_dcoefs, dweight accumulated into or None, dstyles added to) per layer."""
    for i in range(0, len(layers), DEMOD_GROUP_MAX):
        chunk = layers[i:i + DEMOD_GROUP_MAX]
        core.check(core.lib().ldetr_demod_group_bwd_f32(_demod_descs(chunk, grads[i:i + DEMOD_GROUP_MAX]), len(chunk), B, 1, 1, core.stream()),
                   'demod_group_bwd')


def side_affine_bwd(ws, layers):
    """layers: (ds [B, C], affine weight [C, D], dA accumulated into or None, db accumulated into or None, weight gain, post factor) -> dws [B, D]."""
    ws = core.f32c(ws)
    B, D = ws.shape
    dws = torch.empty((B, D), device=ws.device, dtype=torch.float32)
    for i in range(0, len(layers), AFFINE_GROUP_MAX):
        chunk = layers[i:i + AFFINE_GROUP_MAX]
        descs = (_lib.AffineDesc * len(chunk))()
        floats = 0
        for d, (ds, A, dA, db, gain, post) in zip(descs, chunk):
            d.ds, d.A = ds.data_ptr(), A.data_ptr()
            d.dA, d.db = (dA.data_ptr() if dA is not None else None), (db.data_ptr() if db is not None else None)
            d.C, d.scale, d.post = A.shape[0], gain * post, post
            floats += (A.shape[0] + 63) // 64 * B * D
        scratch = torch.empty(floats, device=ws.device, dtype=torch.float32)
        core.check(core.lib().ldetr_sg2_affine_bwd_f32(descs, len(chunk), core.ptr(ws), core.ptr(dws), 1 if i else 0, core.ptr(scratch), floats, B, D,
                                                       core.stream()), 'sg2_affine_bwd')
    return dws


def _torgb_fwd(x, w, s, b, img):
    """toRGB of a block; `img` (the upsampled image of the block below, or None) is added by the same launch when the streaming kernel applies."""
    B, H, W, C = x.shape
    c4 = C // 4
    if img is None or not (C % 4 == 0 and C <= 512 and (c4 & (c4 - 1)) == 0 and s.stride(0) == C):
        y = modconv.torgb_fwd(x, w, s, b)
        return img + y if img is not None else y
    img = img.contiguous()
    y = torch.empty((B, H, W, 3), device=x.device, dtype=torch.float32)
    core.check(core.lib().ldetr_torgb_fwd_add_f32(core.ptr(x), core.ptr(w), core.ptr(s), core.ptr(b), core.ptr(img), core.ptr(y), B, H * W, C, core.stream()),
               'torgb_fwd_add')
    return y


class _SynthesisFn(torch.autograd.Function):
    """forward(blocks, const, f, *tensors) -> image NHWC [B, R, R, 3].  tensors, per block from 4x4 up:
    [conv0: weight, bias, styles, dcoefs]  conv1: weight, bias, styles, dcoefs  torgb: weight, bias, styles (weight gain included).
    With the side chain inside (blocks[i].affines set): the latent ws [B, w_dim] first, then per block
    [conv0: weight, bias, affine weight, affine bias]  conv1: the same four  torgb: the same four."""

    @staticmethod
    def forward(ctx, blocks, const, f, *tensors):
        core.require_gpu(const, f, *tensors)
        keep = any(ctx.needs_input_grad)         # under no_grad (G_ema, generation) nothing is kept
        side = blocks[0].affines is not None
        ws = None
        if side:
            ws, tensors = tensors[0], tensors[1:]
            if not (ws.dtype == torch.float32 and ws.stride(1) == 1 and ws.stride(0) >= ws.shape[1] and ws.stride(0) % 4 == 0 and ws.data_ptr() % 16 == 0):
                ws = core.f32c(ws)               # (the operand conditions of linear(): a pitched latent goes to the GEMM as it is)
            # the side chain: every style, then every coefficient set, in the tensors' order
            kinds = [k for blk in blocks for k in (('conv0',) if blk.has_conv0 else ()) + ('conv1', 'torgb')]
            affs = [blk.affines[k] for blk in blocks for k in (('conv0',) if blk.has_conv0 else ()) + ('conv1', 'torgb')]
            affs = [(core.f32c(tensors[4 * i + 2].detach()), core.f32c(tensors[4 * i + 3].detach()), a[2], a[3]) for i, a in enumerate(affs)]
            styles = side_styles(ws, affs)
            convs = [i for i, k in enumerate(kinds) if k != 'torgb']
            wdet = [tensors[4 * i].detach() if tensors[4 * i].dtype == torch.float32 else tensors[4 * i].detach().float() for i in convs]
            dcoefs, w2s = side_demod(wdet, [styles[i] for i in convs])
            side_of = {i: (wdet[j], dcoefs[j], w2s[j]) for j, i in enumerate(convs)}
        it = iter(tensors)
        saved, layout = [const, f], []
        x = img = None
        B = ws.shape[0] if side else tensors[2].shape[0]
        li = 0                                   # running layer index (side chain)

        def layer(is_conv):
            nonlocal li
            if not side:
                return [next(it) for _ in range(4 if is_conv else 3)] + [None]
            w, b = next(it), next(it)
            next(it); next(it)
            rec = (li, side_of[li][0], side_of[li][2], affs[li][0]) if is_conv else (li, affs[li][0])
            out = [w, b, styles[li]] + ([side_of[li][1]] if is_conv else []) + [rec]
            li += 1
            return out
        for blk in blocks:
            entry = {}
            if blk.has_conv0:
                w, b, s, d, extra = layer(True)
                w = core.f32c(weight_ohwi(w)); b = core.f32c(b); s = core.f32c(s); d = core.f32c(d)
                _, x0 = modconv.up_fwd(x, w, s, d, b, f, ACT_ALPHA, blk.gains[0])
                entry['conv0'] = (w, b, s, d, x0)
                if side:
                    entry['side_conv0'] = extra[1:]
                x = x0
            else:
                x = core.f32c(const).permute(1, 2, 0).unsqueeze(0).repeat([B, 1, 1, 1])
                entry['xin'] = (x,)
            w, b, s, d, extra = layer(True)
            w = core.f32c(weight_ohwi(w)); b = core.f32c(b); s = core.f32c(s); d = core.f32c(d)
            x = modconv.conv_fwd(x, w, s, d, b, w.shape[1] // 2, ACT_ALPHA, blk.gains[1])
            entry['conv1'] = (w, b, s, d, x)
            if side:
                entry['side_conv1'] = extra[1:]
            if img is not None:
                # upfirdn2d.upsample2d with the 4-tap filter: up 2, pad [2, 1, 2, 1], gain 4
                img = _up._kernel_call(img.permute(0, 3, 1, 2), f, 2, 2, 1, 1, 2, 1, 2, 1, False, 4.0).permute(0, 2, 3, 1)
            w, b, s, extra = layer(False)
            ctx_wshape = w.shape
            w = core.f32c(w.reshape(w.shape[0], -1)); b = core.f32c(b); s = core.f32c(s)
            if w.shape[0] != 3:
                raise NotImplementedError('the synthesis node is specialised for 3 colour channels')
            if side:
                img = _torgb_fwd(x, w, s, b, img)
                entry['side_torgb'] = extra[1:]
            else:
                y = modconv.torgb_fwd(x, w, s, b)
                img = img + y if img is not None else y
            entry['torgb'] = (w, s)
            entry['rgb_wshape'] = ctx_wshape
            if keep:
                rec = {}
                for k in ('conv0', 'xin', 'conv1', 'torgb', 'side_conv0', 'side_conv1', 'side_torgb'):
                    if k in entry:
                        rec[k] = (len(saved), len(entry[k]))
                        saved += list(entry[k])
                rec['rgb_wshape'] = ctx_wshape
                layout.append(rec)
        if keep:
            if side:
                saved.append(ws)
            ctx.save_for_backward(*saved)
            ctx.blocks, ctx.layout, ctx.side = blocks, layout, side
        return img

    @staticmethod
    def backward(ctx, dimg):
        saved = ctx.saved_tensors
        const, f = saved[0], saved[1]
        blocks, layout, side = ctx.blocks, ctx.layout, ctx.side
        per = 4 if side else 3                   # tensors of a toRGB; a conv has 4 either way
        need = ctx.needs_input_grad[(4 if side else 3):]
        get = lambda rec, k: saved[rec[k][0]:rec[k][0] + rec[k][1]]
        dimg = core.f32c(dimg)
        dev = dimg.device
        grads = [None] * len(need)
        # position of each block's first tensor in `tensors`
        first, n = [], 0
        for blk in blocks:
            first.append(n)
            n += (8 if blk.has_conv0 else 4) + per
        ds_of, dd_of = {}, {}                    # position of a layer's first tensor -> its style / demodulation gradient
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
                ds_of[first[i + 1]] = ds_next
            grads[o + 4] = None if wr_flat else dw_rgb.reshape(rec['rgb_wshape'])
            grads[o + 5] = None if br_flat else dbias_rgb
            ds_of[o + 4] = ds_rgb
            grads[o + 1] = None if b1_flat else db1
            dd_of[o] = dd1
            # conv1
            xin = get(rec, 'conv0')[4] if blk.has_conv0 else get(rec, 'xin')[0]
            pad = w1.shape[1] // 2
            dxs1 = modconv.conv_bwd_data(dv1, w1, d1, B, xin.shape[1], xin.shape[2], pad)
            if need[o]:
                grads[o] = modconv.conv_bwd_weight(xin, dv1, w1, s1, d1, w1p, pad)
            if not blk.has_conv0:
                # the 4x4 block: its input is the constant, expanded over the batch
                dx, ds1 = modconv._mul_reduce(dxs1, xin, s1, B, xin.shape[1] * xin.shape[2], xin.shape[3])
                ds_of[o] = ds1
                if ctx.needs_input_grad[1]:
                    dconst = dx.sum(0).permute(2, 0, 1)
                break
            # hand-off conv1 -> conv0, FIR adjoint, transposed conv
            w0, b0, s0, d0, x0 = get(rec, 'conv0')
            w0p, b0p = blk.params['conv0']
            db0, b0_flat = _bias_target(b0p, C, dev)
            dv0, ds1, _, dd0 = _handoff(dxs1, x0, None, s1, None, b0, d0, db0, blk.gains[0])
            ds_of[o] = ds1
            grads[first[i] + 1] = None if b0_flat else db0
            dd_of[first[i]] = dd0
            dud = modconv.up_fir_adjoint(dv0, f)
            xprev = get(layout[i - 1], 'conv1')[4]
            dxs_next = modconv.up_bwd_data(dud, w0, d0, B, xprev.shape[1], xprev.shape[2])
            s_next = s0
            if need[first[i]]:
                grads[first[i]] = modconv.up_bwd_weight(xprev, dud, w0, s0, d0, w0p)
            # adjoint of upsample2d on the 3-channel image gradient: down 2, pad [1, 1, 1, 1], flipped taps, gain 4
            dimg = _up._kernel_call(dimg.permute(0, 3, 1, 2), f, 1, 1, 2, 2, 1, 1, 1, 1, True, 4.0).permute(0, 2, 3, 1)
        if not side:
            for p, t in ds_of.items():
                grads[p + 2] = t
            for p, t in dd_of.items():
                grads[p + 3] = t
            return (None, dconst, None) + tuple(grads)
        dws = _SynthesisFn._side_backward(ctx, saved, blocks, layout, first, need, grads, ds_of, dd_of)
        return (None, dconst, None, dws) + tuple(grads)

    @staticmethod
    def _side_backward(ctx, saved, blocks, layout, first, need, grads, ds_of, dd_of):
        """The side chain's backward, after every style and demodulation gradient exists: the grouped demodulation backward (weight part into
        the conv weights' gradients, style part added to ds), then the affines' backward.  -> the latent's gradient; fills `grads`."""
        get = lambda rec, k: saved[rec[k][0]:rec[k][0] + rec[k][1]]
        ws = saved[-1]
        B = ws.shape[0]
        demod_layers, demod_grads, aff_layers, fix = [], [], [], []
        for i, (blk, rec) in enumerate(zip(blocks, layout)):
            names = (('conv0', first[i]),) if blk.has_conv0 else ()
            names += (('conv1', first[i] + (4 if blk.has_conv0 else 0)), ('torgb', first[i] + (8 if blk.has_conv0 else 4)))
            for name, p in names:
                ds = ds_of[p]
                extra = get(rec, 'side_' + name)
                if name != 'torgb':
                    wdet, w2, aw = extra
                    _, _, s, d, _ = get(rec, name)
                    dwt = None
                    if need[p]:
                        acc = core.flat_grad(blk.params[name][0])
                        if acc is not None and acc.stride() == wdet.stride():
                            dwt = acc
                        else:      # no flat gradient view: the demodulation path's share joins the convolution's through an add
                            dwt = torch.zeros_like(wdet)
                            fix.append((p, dwt))
                    demod_layers.append((wdet, s, d, w2))
                    demod_grads.append((dd_of[p], dwt, ds))
                else:
                    aw, = extra
                aparam, bparam, gain, post = blk.affines[name]
                dA = db = None
                if need[p + 2]:
                    dA = core.flat_grad(aparam)
                    if dA is None or not dA.is_contiguous():
                        dA = torch.zeros_like(aw)
                        grads[p + 2] = dA
                if need[p + 3]:
                    db = core.flat_grad(bparam)
                    if db is None or not db.is_contiguous():
                        db = torch.zeros(aw.shape[0], device=aw.device, dtype=torch.float32)
                        grads[p + 3] = db
                aff_layers.append((ds, aw, dA, db, gain, post))
        side_demod_bwd(demod_layers, demod_grads, B)
        for p, dwt in fix:
            grads[p] = dwt if grads[p] is None else grads[p] + dwt
        return side_affine_bwd(ws, aff_layers)


def run(blocks, const, f, tensors):
    """-> image NHWC [B, R, R, 3]."""
    NODE_RUNS[0] += 1
    return _SynthesisFn.apply(blocks, const, f, *tensors)
