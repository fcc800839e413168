"""What tests/test_resampling_ref_cpu.py and tests/test_resampling_gpu.py share for the FIR resampling kernels (csrc/upfirdn2d.hip behind
torch_utils/ops/upfirdn2d.py), the demodulation coefficients (csrc/demod.hip behind hip/modconv.py) and the page resize (csrc/resample.hip behind
training/dataset_layoutganpp.py): float64 references, the case tables, and one predicate per family that restates the host-side selection and names
the paths a case takes.  The CPU file asserts that every path name is reached by a table case; the GPU file runs the tables.  Nothing here touches
the GPU or the kernel library.

Every reference takes `dtype`: float64 is the reference, float32 is the yardstick (the same formula evaluated by torch on the CPU in the kernels'
number format; for demod the kernel's own W2 formula).  FP32_BASELINE holds those float32 errors as measured over the tables, the GPU file allows
4 x them (other summation order, fma contraction, rsqrtf) but never more than the project's older figures, and the CPU file re-measures them and
asserts that each recorded figure is within a factor 4 of what it finds.

Inputs are chosen so that the element-wise measure means something.  The rounding inputs of upfirdn2d are positive (x, the upstream gradient and
every tap), and so is the upstream gradient of demod, whose sums are then sums of terms of one sign: no output is the small difference of large
terms, every element can be compared relatively, and an output whose window lies in the padding or between the inserted zeros is exactly 0 on
both sides.  Signs are the business of the exact inputs (integers in [-8, 8], dyadic taps: every partial sum is a float32, so the result does not
depend on the order of summation and must equal the float64 reference) and of the fused-epilogue cases, which are signed and measured max-normalised
only.

The gain: ops_ref.upfirdn2d multiplies a 1-D filter by gain ** 0.5 for each of its two passes, which is not a float for gain 1.5; upfirdn_ref runs
it with gain 1 and multiplies the result, the same number without that rounding, so that the exact check holds for the separable filter too."""
import functools
import itertools
import os

import numpy as np
import torch

from oracle import ops_ref, resample_ref

F64, F32 = torch.float64, torch.float32


def limit_threads():
    """CPU references: more threads than this are slower on many-core hosts."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def rel_err(a, b):
    """max |a - b| / max |b|, the suite's measure."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def elem_rel_err(a, b):
    """max over elements of |a - b| / |b|; an element whose reference is exactly 0 must be exactly 0."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    zero = b == 0
    if not bool((a[zero] == 0).all()):
        return float('inf')
    if bool(zero.all()):
        return 0.0
    return ((a - b).abs()[~zero] / b.abs()[~zero]).max().item()


def as_f32(v):
    """A scalar argument as the kernel receives it: rounded to float32."""
    return float(torch.tensor(v, dtype=F32))


# Bounds the project already has, in rel_err's measure (tests/test_kernels_gpu.py: test_upfirdn2d*, test_demod_coefficients_fwd_bwd).
PROJECT_BOUND = dict(upfirdn_y=3e-6, upfirdn_dx=3e-6, upfirdn_act=3e-6, upfirdn_ddy=3e-6, demod_d=5e-6, demod_dw=2e-5, demod_ds=2e-5)

# float32 torch on the CPU against the float64 reference, worst case over the tables below (test_resampling_ref_cpu.py re-measures them); the GPU
# file allows FP32_FACTOR x these and at most PROJECT_BOUND.  upfirdn_y, upfirdn_dx: forward and input gradient of every table case with the
# positive rounding inputs (rel_err; *_elem: elem_rel_err);  upfirdn_act: the fused-epilogue cases, signed;  upfirdn_ddy: the second-order case;
# demod_*: the kernel's W2 formula in float32 (dcoefs, dweight, dstyles).
FP32_BASELINE = dict(upfirdn_y=2.37e-7, upfirdn_y_elem=3.69e-7, upfirdn_dx=2.54e-7, upfirdn_dx_elem=3.65e-7, upfirdn_act=1.73e-7, upfirdn_ddy=1.12e-7,
                     demod_d=3.86e-7, demod_d_elem=4.90e-7, demod_dw=4.43e-7, demod_dw_elem=1.03e-6, demod_ds=7.91e-7, demod_ds_elem=1.15e-6)
FP32_FACTOR = 4.0      # -> bounds 9.5e-7, 1.5e-6, 1.0e-6, 1.5e-6, 6.9e-7, 4.5e-7; 1.5e-6, 2.0e-6, 1.8e-6, 4.1e-6, 3.2e-6, 4.6e-6


def fp32_bound(key):
    b = FP32_FACTOR * FP32_BASELINE[key]
    return min(b, PROJECT_BOUND[key]) if key in PROJECT_BOUND else b


# ------------------------------------------------------------------------------------------------------------------------ upfirdn2d
UF_GRID_CAP = 256 * 32        # csrc/upfirdn2d.hip:280
UF_FIR_MIN_OUT = 64           # :281
UF_FIR_BIG = 1 << 20          # :286
UF_XCD_MIN_BLOCKS = 64        # :290
ACT_ALPHA, ACT_GAIN = 0.25, 2.0

FILTERS = ['4x4', 'sep8', '1x1', 'none']
PADS = dict(layer=(1, 1, 1, 1), adjoint=(2, 2, 2, 2), mixed=(3, 0, -1, 2), crop=(-2, 1, -1, 2))        # (px0, px1, py0, py1)
UPDOWN = [((1, 1), (1, 1)), ((2, 2), (1, 1)), ((1, 1), (2, 2)), ((2, 1), (1, 3)), ((3, 2), (2, 3)), ((1, 3), (3, 1))]       # ((upx, upy), (downx, downy))
GAINS = [4.0, 1.5]
# 'cl' = channels_last; '_offset1' = the same view one float into its buffer; '_sliced' = a view that leaves out a border of a larger tensor;
# '_expanded' = one sample expanded over the batch (stride 0)
LAYOUTS = ['nchw', 'cl', 'cl_offset1', 'nchw_sliced', 'cl_sliced', 'nchw_expanded']
BASE_SHAPE = (2, 8, 12, 13)
BASE_SHAPE_C6 = (2, 6, 12, 13)


def make_filter(kind, exact):
    """The FIR taps of a case (float32, as the wrapper receives them).  exact: dyadic taps; both forms are asymmetric, so a flip is seen."""
    if kind == 'none':
        return None
    if kind == '1x1':
        return torch.tensor([[0.75]])
    if kind == '4x4':
        if exact:
            return (torch.outer(torch.tensor([1., 3., 3., 1.]), torch.tensor([1., 3., 3., 1.])) + torch.arange(16.).reshape(4, 4)) / 64.0
        return ops_ref.setup_filter([1, 3, 3, 1]) + 0.01 * torch.arange(16.).reshape(4, 4)       # the filter of test_upfirdn2d
    if kind == 'sep8':
        return torch.tensor([1., 2., 4., 9., 8., 5., 2., 1.]) / 32.0 if exact else torch.tensor([1., 2., 4., 7., 6., 5., 2., 1.]) / 28.0
    raise KeyError(kind)


def filter_size(kind):
    """-> (fw, fh) as torch_utils/ops/upfirdn2d.py:32-36."""
    return dict([('4x4', (4, 4)), ('sep8', (8, 8)), ('1x1', (1, 1)), ('none', (1, 1))])[kind]


def uf_case(name, shape, layout='nchw', filt='4x4', up=(1, 1), down=(1, 1), pad=(1, 1, 1, 1), flip=False, gain=4.0, act=None, via='wrapper', seed=0):
    """act: None, 'bias' or 'nobias' (the fused epilogue, C entry only).  via: 'wrapper' = upfirdn2d.upfirdn2d, 'abi' = ldetr_upfirdn2d_f32
    called by the test with a prefilled output and a guard band."""
    assert layout in LAYOUTS and filt in FILTERS and act in (None, 'bias', 'nobias') and via in ('wrapper', 'abi')
    assert act is None or via == 'abi'
    return dict(name=name, shape=tuple(shape), layout=layout, filt=filt, up=tuple(up), down=tuple(down), pad=tuple(pad), flip=bool(flip),
                gain=float(gain), act=act, via=via, seed=seed)


def dense_strides(shape, cl):
    N, C, H, W = shape
    return (C * H * W, 1, W * C, C) if cl else (C * H * W, H * W, W, 1)


def layout_geometry(shape, layout):
    """-> (buffer shape NCHW, buffer channels_last?, storage offset in floats, strides NCHW of the view) of an input as build_input makes it."""
    N, C, H, W = shape
    cl = layout.startswith('cl')
    if layout in ('nchw', 'cl'):
        return shape, cl, 0, dense_strides(shape, cl)
    if layout == 'cl_offset1':
        return shape, cl, 1, dense_strides(shape, cl)
    if layout in ('nchw_sliced', 'cl_sliced'):      # big[:, :, 1:, 2:] of a tensor with one more row and two more columns
        big = (N, C, H + 1, W + 2)
        st = dense_strides(big, cl)
        return big, cl, st[2] + 2 * st[3], st
    if layout == 'nchw_expanded':
        st = dense_strides((1, C, H, W), False)
        return (1, C, H, W), False, 0, (0,) + st[1:]
    raise KeyError(layout)


def build_input(x, layout):
    """x: dense NCHW values (any device, any dtype; for 'nchw_expanded' every sample equals the first) -> a tensor of the same values in the
    memory layout `layout`, cut from a NaN-filled buffer where the layout leaves memory out."""
    shape = tuple(x.shape)
    big, cl, off, st = layout_geometry(shape, layout)
    if layout == 'nchw':
        return x.contiguous()
    if layout == 'cl':
        return x.contiguous(memory_format=torch.channels_last)
    if layout == 'nchw_expanded':
        return x[0:1].contiguous().expand(shape)
    if layout == 'cl_offset1':
        # 3 floats of slack in front: the buffer is 16-byte aligned, the view starts 4 bytes past a 16-byte boundary
        buf = torch.full((x.numel() + 4,), float('nan'), dtype=x.dtype, device=x.device)
        v = buf.as_strided(shape, st, 1)
        v.copy_(x)
        return v
    buf = torch.full(big, float('nan'), dtype=x.dtype, device=x.device)
    if cl:
        buf = buf.contiguous(memory_format=torch.channels_last)
    v = buf[:, :, 1:, 2:]
    v.copy_(x)
    return v


def out_size(n, up, p0, p1, taps, down):
    return (n * up + p0 + p1 - taps + down) // down


def uf_launches(c):
    """The kernel launches of a case's forward as torch_utils/ops/upfirdn2d.py:100-111 and _kernel_call (:60-84) make them: one for a 2-D filter
    (None is a 1 x 1 of ones), two for a 1-D one (along x with gain 1, then along y); the output is channels_last when x.stride(1) == 1 and C > 1."""
    N, C, H, W = c['shape']
    _, _, x_off, xs = layout_geometry(c['shape'], c['layout'])
    (upx, upy), (dnx, dny), (px0, px1, py0, py1) = c['up'], c['down'], c['pad']
    fw, fh = filter_size(c['filt'])

    def one(xs, x_off, H, W, fw, fh, upx, upy, dnx, dny, px0, px1, py0, py1):
        oW, oH = out_size(W, upx, px0, px1, fw, dnx), out_size(H, upy, py0, py1, fh, dny)
        assert oW >= 1 and oH >= 1, c['name']
        ys = dense_strides((N, C, oH, oW), xs[1] == 1 and C > 1)
        return dict(N=N, C=C, inH=H, inW=W, outH=oH, outW=oW, xs=xs, x_off=x_off, ys=ys, y_off=0, up=(upx, upy), down=(dnx, dny), fw=fw, fh=fh,
                    pad0=(px0, py0), act=c['act'])
    if c['filt'] != 'sep8':
        return [one(xs, x_off, H, W, fw, fh, upx, upy, dnx, dny, px0, px1, py0, py1)]
    first = one(xs, x_off, H, W, fw, 1, upx, 1, dnx, 1, px0, px1, 0, 0)
    return [first, one(first['ys'], 0, H, first['outW'], 1, fh, 1, upy, 1, dny, 0, 0, py0, py1)]


def launch_paths(L):
    """ldetr_upfirdn2d_f32's selection (csrc/upfirdn2d.hip:275-293) and what the chosen kernel does with the shape -> set of path names."""
    N, C, oH, oW, xs, ys = L['N'], L['C'], L['outH'], L['outW'], L['xs'], L['ys']
    aligned = L['x_off'] % 4 == 0 and L['y_off'] % 4 == 0
    strides4 = all(s % 4 == 0 for s in (xs[3], xs[2], xs[0], ys[3], ys[2], ys[0]))
    nhwc4 = xs[1] == 1 and ys[1] == 1 and C % 4 == 0 and aligned and strides4                       # :275-277
    names = set()
    if not nhwc4:
        total = N * C * oH * oW
        names |= {'planar', 'planar/' + ('stride_loop' if total > UF_GRID_CAP * 256 else 'single_round')}      # :279-280, the loop of :63
        if xs[1] != 1 or ys[1] != 1:
            names.add('planar/nchw' if xs == dense_strides((N, C, L['inH'], L['inW']), False) else 'planar/strided_view')
        elif C % 4:
            names.add('planar/cl_c_not_mult4')
        elif not aligned:
            names.add('planar/cl_misaligned')
        else:
            names.add('planar/strided_view')
        return names
    quads = N * oH * oW * (C // 4)
    if not (L['up'] == (1, 1) and L['down'] == (1, 1) and L['fw'] == 4 and L['fh'] == 4 and oH * oW >= UF_FIR_MIN_OUT):      # :281
        names |= {'nhwc4', 'nhwc4/' + ('stride_loop' if quads > UF_GRID_CAP * 256 else 'single_round')}
        if L['act']:
            names.add('nhwc4/act_' + L['act'])
        return names
    TR = 8 if quads >= UF_FIR_BIG else 4                                                                  # :286-287
    threads = N * ((oH + TR - 1) // TR) * ((oW + 1) // 2) * (C // 4)                                      # :288
    g = (threads + 255) // 256
    names.add(f'fir4x4/TR{TR}')
    if g >= UF_XCD_MIN_BLOCKS:                                                                            # :290
        names.add('fir4x4/xcd_map/full' if g % 8 == 0 else 'fir4x4/xcd_map/padded_grid')
    else:
        names.add('fir4x4/identity_map')
    if oW % 2:
        names.add('fir4x4/ragged_right')                                                                  # :233
    if oH % TR:
        names.add('fir4x4/ragged_bottom')                                                                 # :224
    if threads % 256:
        names.add('fir4x4/partial_block')                                                                 # :169
    if L['pad0'][0] < 0 or L['pad0'][1] < 0:
        names.add(f'fir4x4/TR{TR}/crop')                                                                  # :178, ix0 / iy0 positive
    if L['act']:
        names.add('fir4x4/act_' + L['act'])                                                               # :190-191, :228-232
    return names


def upfirdn_paths(c):
    out = set()
    for L in uf_launches(c):
        out |= launch_paths(L)
    return out


UPFIRDN_PATHS = ['planar', 'nhwc4', 'fir4x4/TR4', 'fir4x4/TR8', 'planar/single_round', 'planar/stride_loop', 'nhwc4/single_round', 'nhwc4/stride_loop',
                 'fir4x4/identity_map', 'fir4x4/xcd_map/full', 'fir4x4/xcd_map/padded_grid', 'fir4x4/ragged_right', 'fir4x4/ragged_bottom',
                 'fir4x4/partial_block', 'fir4x4/TR4/crop', 'fir4x4/TR8/crop', 'fir4x4/act_bias', 'fir4x4/act_nobias', 'nhwc4/act_bias', 'nhwc4/act_nobias',
                 'planar/nchw', 'planar/cl_c_not_mult4', 'planar/cl_misaligned', 'planar/strided_view']


def _uf_cross():
    """flip x gain x pad x up/down x filter in full; the memory layout (and with it the kernel) rotates through the product: 7 forms against
    factor counts of 2, 2, 4, 6 and 4, so every pair (layout, value of a factor) occurs."""
    forms = [('nchw', BASE_SHAPE), ('cl', BASE_SHAPE), ('cl', BASE_SHAPE_C6), ('cl_offset1', BASE_SHAPE), ('nchw_sliced', BASE_SHAPE),
             ('cl_sliced', BASE_SHAPE), ('nchw_expanded', BASE_SHAPE)]
    out = []
    for ud, filt in itertools.product(range(len(UPDOWN)), FILTERS):
        for pad, flip, gain in itertools.product(PADS, (False, True), GAINS):
            layout, shape = forms[len(out) % len(forms)]
            up, down = UPDOWN[ud]
            out.append(uf_case(f'x-ud{ud}-{filt}-{pad}-flip{int(flip)}-g{gain}-{layout}-c{shape[1]}', shape, layout, filt, up, down, PADS[pad], flip, gain,
                               seed=len(out)))
            out[-1]['group'] = f'cross-ud{ud}-{filt}'
    return out


def _uf_special():
    cl64 = lambda H, W: (1, 64, H, W)
    up2 = dict(up=(2, 2), pad=(2, 1, 2, 1))
    cases = [
        # the dispatch boundary outH * outW >= 64: an 8 x 8 output against a 7 x 9 one
        uf_case('fir-boundary-8x8', (1, 8, 9, 9), 'cl', via='abi', seed=500),
        uf_case('fir-boundary-7x9', (1, 8, 8, 10), 'cl', via='abi', seed=501),
        # 64 blocks: the XCD map with a full grid; 66 blocks padded to 72
        uf_case('fir-xcd-full', cl64(129, 65), 'cl', via='abi', gain=1.5, seed=502),
        uf_case('fir-xcd-padded', cl64(131, 65), 'cl', via='abi', flip=True, seed=503),
        uf_case('fir-xcd-padded-act-nobias', cl64(131, 65), 'cl', via='abi', gain=1.5, act='nobias', seed=504),
        # TR = 8: 257 x 257 (ragged right and bottom), and with a crop on the left and top
        uf_case('fir-tr8-ragged', cl64(258, 258), 'cl', via='abi', seed=505),
        uf_case('fir-tr8-crop', cl64(260, 261), 'cl', via='abi', pad=PADS['crop'], flip=True, gain=1.5, seed=506),
        # past the capped grid
        uf_case('planar-stride-loop', (1, 3, 841, 841), 'nchw', via='abi', seed=507),
        uf_case('nhwc4-stride-loop', (1, 8, 513, 513), 'cl', via='abi', seed=508, **up2),
        # the fused epilogue on each kernel, with and without a bias
        uf_case('fir-act-bias', BASE_SHAPE, 'cl', via='abi', act='bias', seed=509),
        uf_case('fir-act-nobias', BASE_SHAPE, 'cl', via='abi', act='nobias', flip=True, seed=510),
        uf_case('fir-act-bias-adjoint-pad', (2, 8, 11, 12), 'cl', via='abi', act='bias', pad=PADS['adjoint'], flip=True, seed=511),
        uf_case('nhwc4-act-bias', BASE_SHAPE, 'cl', via='abi', act='bias', seed=512, **up2),
        uf_case('nhwc4-act-nobias', BASE_SHAPE, 'cl', via='abi', act='nobias', gain=1.5, seed=513, **up2),
        uf_case('planar-act-bias', BASE_SHAPE_C6, 'cl', via='abi', act='bias', seed=514),
        uf_case('planar-act-bias-nchw', BASE_SHAPE, 'nchw', via='abi', act='bias', seed=515, **up2),
    ]
    for c in cases:
        c['group'] = c['name']
    return cases


UPFIRDN_CASES = _uf_cross() + _uf_special()
UPFIRDN_BY_NAME = {c['name']: c for c in UPFIRDN_CASES}
assert len(UPFIRDN_BY_NAME) == len(UPFIRDN_CASES)
UPFIRDN_GROUPS = list(dict.fromkeys(c['group'] for c in UPFIRDN_CASES))
# the same data through fir4x4 (channels_last) and through the planar kernel (the same view one float into its buffer), power-of-two gain
BIT_IDENTITY_CASES = [uf_case('bits-small', BASE_SHAPE, 'cl', seed=600), uf_case('bits-small-flip-adjoint', BASE_SHAPE, 'cl', pad=PADS['adjoint'], flip=True, seed=601),
                      uf_case('bits-xcd-padded', (1, 64, 131, 65), 'cl', gain=2.0, seed=602), uf_case('bits-crop', BASE_SHAPE, 'cl', pad=PADS['crop'], gain=0.5, seed=603)]
SECOND_ORDER_CASE = uf_case('second-order', BASE_SHAPE, 'cl', up=(2, 1), down=(1, 3), pad=PADS['mixed'], gain=1.5, seed=610)
# filter2d / upsample2d / downsample2d (torch_utils/ops/upfirdn2d.py:141-161): (helper, filter, factor, padding, flip, gain)
HELPER_CASES = [('filter2d', '4x4', None, 0, False, 1.0), ('filter2d', 'sep8', None, [1, 0, -1, 2], True, 1.5), ('upsample2d', '4x4', 2, 0, False, 1.0),
                ('upsample2d', 'sep8', [3, 2], [0, 1, 1, 0], True, 1.0), ('downsample2d', '4x4', 2, 0, False, 1.0), ('downsample2d', 'sep8', [2, 3], 1, True, 1.5),
                ('downsample2d', 'none', 2, 0, False, 1.0)]


def uf_inputs(c, exact):
    """-> x [N, C, H, W], bias [C] or None (float32).  exact: integers in [-8, 8]; else positive (signed for the fused epilogue, see the module
    docstring).  For 'nchw_expanded' every sample is the first."""
    gen = torch.Generator().manual_seed(20000 + c['seed'] * 2 + int(exact))
    if exact:
        x = torch.randint(-8, 9, c['shape'], generator=gen).float()
    elif c['act']:
        x = torch.randn(c['shape'], generator=gen)
    else:
        x = torch.randn(c['shape'], generator=gen).abs() + 0.1
    if c['layout'] == 'nchw_expanded':
        x = x[0:1].expand(c['shape']).contiguous()
    bias = None
    if c['act'] == 'bias':
        bias = torch.randint(-8, 9, (c['shape'][1],), generator=gen).float() if exact else torch.randn(c['shape'][1], generator=gen)
    return x, bias


def uf_upstream(c, shape, exact):
    gen = torch.Generator().manual_seed(40000 + c['seed'] * 2 + int(exact))
    return torch.randint(-8, 9, shape, generator=gen).float() if exact else torch.randn(shape, generator=gen).abs() + 0.1


def upfirdn_ref(x, f, up, down, pad, flip, gain, bias=None, act=None, dtype=F64):
    """oracle.ops_ref.upfirdn2d in `dtype` (gain applied to its result, see the module docstring), then the fused epilogue
    lrelu(v + bias[c], alpha) * act_gain (csrc/upfirdn2d.hip:48-55)."""
    f = f.to(dtype) if f is not None else torch.ones([1, 1], dtype=dtype)
    y = ops_ref.upfirdn2d(x.to(dtype), f, up=up, down=down, padding=list(pad), flip_filter=flip, gain=1) * gain
    if act:
        if bias is not None:
            y = y + bias.to(dtype).reshape(1, -1, 1, 1)
        y = torch.nn.functional.leaky_relu(y, ACT_ALPHA) * ACT_GAIN
    return y


def upfirdn_direct(x, f, up, down, pad, flip, gain):
    """The definition as four nested loops over output and taps, float64, independent of ops_ref: zero-insert, pad / crop, true convolution (the
    taps reversed) unless flip, decimate.  f: None, [fh, fw] or [taps] (outer product)."""
    x = x.double()
    N, C, H, W = x.shape
    f = torch.ones(1, 1, dtype=F64) if f is None else f.double()
    if f.ndim == 1:
        f = torch.outer(f, f)
    fh, fw = f.shape
    (upx, upy), (dnx, dny), (px0, px1, py0, py1) = up, down, pad
    oW, oH = out_size(W, upx, px0, px1, fw, dnx), out_size(H, upy, py0, py1, fh, dny)
    y = torch.zeros(N, C, oH, oW, dtype=F64)
    for oy in range(oH):
        for ox in range(oW):
            for ky in range(fh):
                for kx in range(fw):
                    uy, ux = oy * dny + ky - py0, ox * dnx + kx - px0          # position in the zero-inserted image
                    if uy % upy or ux % upx or not (0 <= uy // upy < H and 0 <= ux // upx < W):
                        continue
                    tap = f[ky, kx] if flip else f[fh - 1 - ky, fw - 1 - kx]
                    y[:, :, oy, ox] += x[:, :, uy // upy, ux // upx] * tap
    return y * gain


def uf_reference(c, exact, dtype=F64):
    """-> (y, dx, g): forward (with the fused epilogue where the case has one), the upstream gradient (float32) and the input gradient of the
    FIR itself (the epilogue exists on the C entry only, the autograd Function differentiates the FIR) by autograd, dense NCHW in `dtype`."""
    x, bias = uf_inputs(c, exact)
    xr = x.to(dtype).requires_grad_(True)
    f = make_filter(c['filt'], exact)
    lin = upfirdn_ref(xr, f, c['up'], c['down'], c['pad'], c['flip'], c['gain'], dtype=dtype)
    g = uf_upstream(c, lin.shape, exact)
    (dx,) = torch.autograd.grad(lin, xr, g.to(dtype))
    y = upfirdn_ref(x, f, c['up'], c['down'], c['pad'], c['flip'], c['gain'], bias, c['act'], dtype) if c['act'] else lin.detach()
    return y, dx, g


@functools.lru_cache(maxsize=None)
def uf_reference_cached(name, exact):
    """The float64 reference of a table case, computed once and shared (do not write to what it returns)."""
    return uf_reference(UPFIRDN_BY_NAME[name], exact)


def second_order_ref(c, dtype=F64):
    """-> (y, dx, ddy, g, v): dx = d<y, g>/dx with the graph kept, ddy = d<dx, v>/dg, which is the forward operator applied to v."""
    x, _ = uf_inputs(c, False)
    xr = x.to(dtype).requires_grad_(True)
    y = upfirdn_ref(xr, make_filter(c['filt'], False), c['up'], c['down'], c['pad'], c['flip'], c['gain'], dtype=dtype)
    g = uf_upstream(c, y.shape, False)
    gr = g.to(dtype).requires_grad_(True)
    (dx,) = torch.autograd.grad(y, xr, gr, create_graph=True)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(611)).abs() + 0.1
    (ddy,) = torch.autograd.grad(dx, gr, v.to(dtype))
    return y.detach(), dx.detach(), ddy, g, v


def helper_ref(helper, x, f, factor, padding, flip, gain, dtype=F64):
    """filter2d / upsample2d / downsample2d as the reference's torch_utils/ops/upfirdn2d.py:302-310, :340-349, :379-388 derive their pads."""
    px0, px1, py0, py1 = ops_ref._pad4(padding)
    fw, fh = (1, 1) if f is None else (int(f.shape[-1]), int(f.shape[0]))
    if helper == 'filter2d':
        p, up, down = [px0 + fw // 2, px1 + (fw - 1) // 2, py0 + fh // 2, py1 + (fh - 1) // 2], (1, 1), (1, 1)
    elif helper == 'upsample2d':
        up, down = ops_ref._scale2(factor), (1, 1)
        p = [px0 + (fw + up[0] - 1) // 2, px1 + (fw - up[0]) // 2, py0 + (fh + up[1] - 1) // 2, py1 + (fh - up[1]) // 2]
        gain = gain * up[0] * up[1]
    else:
        up, down = (1, 1), ops_ref._scale2(factor)
        p = [px0 + (fw - down[0] + 1) // 2, px1 + (fw - down[0]) // 2, py0 + (fh - down[1] + 1) // 2, py1 + (fh - down[1]) // 2]
    return upfirdn_ref(x, f, up, down, p, flip, gain, dtype=dtype)


# ------------------------------------------------------------------------------------------------------------------------ demod
DEMOD_MAXB = 64               # csrc/demod.hip:28, hip/modconv.py:310
DEMOD_EPS = 1e-8              # hip/modconv.py:286, :312
DEMOD_B = [1, 15, 16, 17, 33, 64, 65]
DEMOD_I = [1, 36, 255, 256, 257, 600]
DEMOD_O = [1, 3, 5, 100]
DEMOD_K = [1, 3]
DEMOD_LAYOUTS = ['oihw', 'cl', 'slice']
DEMOD_REF_MAX = 10_000_000    # elements of the reference's [B, O, I, K, K] product a case may have


def demod_case(B, O, I, K, layout, zero_row=None, seed=0):
    return dict(name=f'B{B}-O{O}-I{I}-K{K}-{layout}' + (f'-zero{zero_row}' if zero_row is not None else ''), B=B, O=O, I=I, K=K, layout=layout,
                zero_row=zero_row, seed=seed)


def _demod_table():
    """B x I in full; O, K and the weight layout rotate through it (O steps down where the reference's product would pass DEMOD_REF_MAX)."""
    out = []
    for B, I in itertools.product(DEMOD_B, DEMOD_I):
        k = len(out)
        o, K, layout = (k + k // 6) % 4, DEMOD_K[(k // 3) % 2], DEMOD_LAYOUTS[k % 3]
        while B * DEMOD_O[o] * I * K * K > DEMOD_REF_MAX:
            o -= 1
        out.append(demod_case(B, DEMOD_O[o], I, K, layout, seed=k))
    extra = [demod_case(17, 5, 257, 3, 'oihw', zero_row=16, seed=100), demod_case(2, 3, 36, 1, 'cl', zero_row=0, seed=101),
             demod_case(16, 100, 600, 3, 'slice', seed=102), demod_case(64, 100, 36, 3, 'cl', seed=103)]
    return out + [c for c in extra if c['name'] not in {o['name'] for o in out}]


DEMOD_CASES = _demod_table()
DEMOD_BY_NAME = {c['name']: c for c in DEMOD_CASES}
assert len(DEMOD_BY_NAME) == len(DEMOD_CASES)


def demod_paths(c):
    """hip/modconv.py:308-313 and csrc/demod.hip.  Forward (:45-67): ceil(B / 16) rounds of 16 samples over one red16, a last round with fewer,
    one or several trips of the 256-thread loop over I (:34, :49).  Backward: demod_bwd_s_kernel's last block along I is partly idle when
    I % 64 (:96, :103), its four lanes over O are unevenly loaded when O % 4 (:105); the GPU test runs every case with the weight gradient stored,
    summed into a non-zero buffer, alone, and with the style gradient alone (:88, :147-154).  B > 64 takes the GEMM form of demod_coefs."""
    if c['B'] > DEMOD_MAXB:
        return {'gemm_form'}
    names = {f'batch_rounds{(c["B"] + 15) // 16}', 'I_le_256' if c['I'] <= 256 else 'I_gt_256', 'dw/store', 'dw/accumulate', 'dw_only', 'ds_only'}
    if c['B'] % 16:
        names.add('partial_last_round')
    if c['I'] % 64:
        names.add('bwd_s/ragged_I')
    if c['O'] % 4:
        names.add('bwd_s/ragged_O')
    if c['zero_row'] is not None:
        names.add('zero_style_row')
    return names


DEMOD_PATHS = [f'batch_rounds{r}' for r in (1, 2, 3, 4)] + ['partial_last_round', 'I_le_256', 'I_gt_256', 'bwd_s/ragged_I', 'bwd_s/ragged_O', 'dw/store',
                                                            'dw/accumulate', 'dw_only', 'ds_only', 'gemm_form', 'zero_style_row']


def demod_inputs(c):
    """-> w [O, I, K, K], s [B, I], g [B, O] (positive, see the module docstring), dw0 (what the accumulating call finds in the gradient buffer)."""
    gen = torch.Generator().manual_seed(60000 + c['seed'])
    B, O, I, K = c['B'], c['O'], c['I'], c['K']
    w = torch.randn(O, I, K, K, generator=gen) * 0.3
    s = torch.randn(B, I, generator=gen)
    if c['zero_row'] is not None:
        s[c['zero_row']] = 0.0
    g = torch.randn(B, O, generator=gen).abs() + 0.1
    return w, s, g, torch.randn(O, I, K, K, generator=gen)


def demod_weight_layout(w, layout):
    """w dense OIHW -> the same values in OIHW memory, channels_last memory, or as a slice [1:O+1, 2:I+2] of a NaN-filled larger tensor
    -> (view, buffer)."""
    if layout == 'oihw':
        v = w.contiguous()
        return v, v
    if layout == 'cl':
        v = w.contiguous(memory_format=torch.channels_last)
        return v, v
    O, I, K, _ = w.shape
    buf = torch.full((O + 2, I + 3, K, K), float('nan'), dtype=w.dtype, device=w.device)
    v = buf[1:O + 1, 2:I + 2]
    v.copy_(w)
    return v, buf


def demod_ref(w, s, g, dtype=F64):
    """The reference's formulation (training/networks_stylegan2.py:57-61) through autograd -> (dcoefs, dweight, dstyles)."""
    w, s = w.to(dtype).requires_grad_(True), s.to(dtype).requires_grad_(True)
    d = ((w[None] * s[:, None, :, None, None]).square().sum([2, 3, 4]) + as_f32(DEMOD_EPS)).rsqrt()
    dw, ds = torch.autograd.grad(d, (w, s), g.to(dtype))
    return d.detach(), dw, ds


def demod_w2_ref(w, s, g, dtype=F64, eps=None):
    """The kernel's formula (csrc/demod.hip:2-9): rsqrt(sum_i s^2 W2 + eps), W2 = sum over taps of w^2, through autograd."""
    w, s = w.to(dtype).requires_grad_(True), s.to(dtype).requires_grad_(True)
    d = (s.square() @ w.square().sum([2, 3]).t() + (as_f32(DEMOD_EPS) if eps is None else eps)).rsqrt()
    dw, ds = torch.autograd.grad(d, (w, s), g.to(dtype))
    return d.detach(), dw, ds


@functools.lru_cache(maxsize=None)
def demod_reference_cached(name):
    w, s, g, _ = demod_inputs(DEMOD_BY_NAME[name])
    return demod_ref(w, s, g)


# ------------------------------------------------------------------------------------------------------------------------ page resize
RS_LDS_BYTES = 48 * 1024      # csrc/resample.hip:21
RS_UNROLLED_TAPS = 32         # :79


def rs_case(name, n, H, W, out_h, out_w, outputs='both', seed=0):
    assert outputs in ('both', 'u8_only', 'chw_only')
    return dict(name=name, n=n, H=H, W=W, out_h=out_h, out_w=out_w, outputs=outputs, seed=seed)


RESIZE_CASES = [
    rs_case('base-odd', 2, 13, 17, 5, 7, seed=1),                      # 1326 bytes: the buffer ends inside a word; rows start at every alignment
    rs_case('base-odd-u8-only', 2, 13, 17, 5, 7, 'u8_only', seed=2),
    rs_case('base-odd-chw-only', 2, 13, 17, 5, 7, 'chw_only', seed=3),
    rs_case('whole-words', 1, 8, 8, 4, 4, seed=4),
    rs_case('batch-of-3', 3, 9, 11, 4, 6, seed=5),
    rs_case('two-x-blocks', 1, 6, 301, 3, 257, seed=6),
    rs_case('two-x-blocks-512', 1, 5, 1030, 2, 512, seed=7),
    rs_case('upscale', 2, 5, 7, 11, 300, seed=8),
    rs_case('taps31', 1, 35, 9, 7, 4, seed=9),                         # H = 5 S: a window of 31, rows of 30 taps
    rs_case('taps33', 1, 36, 9, 7, 4, seed=10),                        # H = 5 S + 1: a window of 33, rows of up to 30 taps
    rs_case('taps33-32-used', 1, 48, 9, 9, 4, seed=15),                # scale 16 / 3: rows of 32 taps
    rs_case('taps31-wide', 2, 35, 270, 7, 260, 'chw_only', seed=11),
    rs_case('taps33-wide', 2, 36, 270, 7, 260, 'u8_only', seed=12),
    rs_case('row-wider-than-lds', 1, 2, 17001, 3, 2, seed=13),          # a 51 kB row segment: read from global memory
    rs_case('row-wider-than-lds-ragged', 2, 3, 16999, 2, 3, seed=14),
]
RESIZE_BY_NAME = {c['name']: c for c in RESIZE_CASES}
RESIZE_PATHS = ['h/staged', 'h/direct', 'lead0', 'lead1', 'lead2', 'lead3', 'last_word/whole', 'last_word/bytewise', 'xblocks1', 'xblocks2', 'v/unrolled',
                'v/loop', 'v/taps31', 'v/taps33', 'u8_only', 'chw_only', 'both', 'upscale', 'out_h_ne_out_w']


def resize_paths(c):
    """ldetr_resize_normalize_u8 (csrc/resample.hip:138-144) and the two kernels.  Horizontal (:36-58): per block of 256 output columns the input
    span is staged in LDS when span + 8 <= lds_bytes, lead = byte offset of the span in its first word, the last word of the whole buffer is
    assembled byte-wise when the buffer ends inside it.  Vertical (:79-88): taps unrolled up to 32.  The tap arithmetic itself is csrc/pil_resample.hpp's."""
    n, H, W, oh, ow = c['n'], c['H'], c['W'], c['out_h'], c['out_w']
    hb, _, _ = resample_ref.precompute_coeffs(W, ow)
    _, _, vks = resample_ref.precompute_coeffs(H, oh)
    scale = W / ow
    support = 3.0 * max(scale, 1.0)
    lds = (int(256.0 * scale + 2.0 * support) + 4) * 3 + 16                                    # :139
    lds_bytes = RS_LDS_BYTES if lds > RS_LDS_BYTES else (lds + 15) // 16 * 16                   # :140
    src_bytes = n * H * W * 3
    xblocks = (ow + 255) // 256
    names = {f'xblocks{xblocks}', 'v/unrolled' if vks <= RS_UNROLLED_TAPS else 'v/loop', c['outputs']}
    if vks in (31, 33):
        names.add(f'v/taps{vks}')
    if oh > H or ow > W:
        names.add('upscale')
    if oh != ow:
        names.add('out_h_ne_out_w')
    bytewise = False
    for bx in range(xblocks):
        x0 = bx * 256
        x1 = min(x0 + 255, ow - 1)
        first, last = int(hb[x0, 0]), int(hb[x1, 0] + hb[x1, 1])                                # :39
        span = (last - first) * 3
        staged = span + 8 <= lds_bytes                                                          # :42
        names.add('h/staged' if staged else 'h/direct')
        for row in range(n * H):
            row_off = (row * W + first) * 3                                                     # :40
            lead = row_off & 3
            if staged:
                names.add(f'lead{lead}')
                words = (lead + span + 3) >> 2                                                  # :46
                bytewise |= row_off - lead + 4 * words > src_bytes                              # :50
    names.add('last_word/bytewise' if bytewise else 'last_word/whole')
    return names


def resize_inputs(c):
    """uint8 [n, H, W, 3]: noise, the upper half of the first image a ramp along x."""
    rng = np.random.default_rng(70000 + c['seed'])
    imgs = rng.integers(0, 256, (c['n'], c['H'], c['W'], 3), dtype=np.uint8)
    imgs[0, : c['H'] // 2] = (np.arange(c['W'])[None, :, None] * 255 // max(c['W'] - 1, 1)).astype(np.uint8)
    return imgs


@functools.lru_cache(maxsize=None)
def resize_reference_cached(name):
    """oracle.resample_ref -> (uint8 [n, out_h, out_w, 3], float32 [n, 3, out_h, out_w])."""
    c = RESIZE_BY_NAME[name]
    imgs = resize_inputs(c)
    u8 = np.stack([resample_ref.resize_antialias_u8(im, c['out_h'], c['out_w']) for im in imgs])
    return u8, np.stack([resample_ref.normalize_chw(u) for u in u8])


# ------------------------------------------------------------------------------------------------------------------------ float32 yardstick
def measure_fp32_baselines():
    """The float32 CPU evaluation of every formula against its float64 evaluation, worst case over the tables -> dict like FP32_BASELINE."""
    out = dict.fromkeys(FP32_BASELINE, 0.0)

    def worst(key, a, b, elem=True):
        out[key] = max(out[key], rel_err(a, b))
        if elem:
            out[key + '_elem'] = max(out[key + '_elem'], elem_rel_err(a, b))
    for c in UPFIRDN_CASES:
        y64, dx64, _ = uf_reference_cached(c['name'], False)
        y32, dx32, _ = uf_reference(c, False, F32)
        if c['act']:
            worst('upfirdn_act', y32, y64, elem=False)
        else:
            worst('upfirdn_y', y32, y64)
        worst('upfirdn_dx', dx32, dx64)
    worst('upfirdn_ddy', second_order_ref(SECOND_ORDER_CASE, F32)[2], second_order_ref(SECOND_ORDER_CASE)[2], elem=False)
    for c in DEMOD_CASES:
        w, s, g, _ = demod_inputs(c)
        d64, dw64, ds64 = demod_reference_cached(c['name'])
        d32, dw32, ds32 = demod_w2_ref(w, s, g, F32)
        worst('demod_d', d32, d64)
        worst('demod_dw', dw32, dw64)
        worst('demod_ds', ds32, ds64)
    return out
