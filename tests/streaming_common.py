"""What tests/test_streaming_ref_cpu.py and tests/test_streaming_kernels_gpu.py share for the element-wise and row-streaming kernels (csrc/optim.hip,
csrc/bias_act.hip, the toRGB and max-pool kernels of csrc/misc_ops.hip): float64 references written from the formulas of include/ldetr_hip.h and the
kernel comments, the case tables, and one predicate per family that restates the host-side selection and names the path a case takes.  The CPU file
asserts that every path name is reached by a table case; the GPU file runs the tables.  Nothing here touches the GPU or the kernel library.

Every reference takes `dtype`: float64 is the reference, float32 is the yardstick for the checks that have no project bound (the same formula
evaluated by torch on the CPU in the kernels' number format).  FP32_BASELINE holds those float32 errors as measured over the tables, the GPU file
allows 4 x them (other summation order, fma contraction), and the CPU file re-measures them and asserts that each recorded figure is within a
factor 4 of what it finds."""
import math
import os

import torch
import torch.nn.functional as F

from oracle import ops_ref

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


# Bounds the project already has, in rel_err's measure.
TOL_BIAS_ACT = dict(y=2e-6, dx=5e-6)                      # test_bias_act
TOL_OPT_P = 1e-6                                          # test_adam_sanitize_ema (p and the EMA)
TOL_TORGB = dict(dx=5e-5, dws=1e-4, dbias=5e-5)           # test_sg2_handoff_gpu.py, the same quantities

# float32 torch on the CPU against the float64 reference, worst case over the tables below (test_streaming_ref_cpu.py re-measures them);
# the GPU file allows FP32_FACTOR x these.
#   adam_m, adam_v: elem_rel_err of the moments after the last step;  adam_p_update: max |p - p64| / max |p64 - p0| (error relative to the
#   size of the update);  torgb_fwd, finish_dw, finish_ds: rel_err.
#   (torch.optim.Adam in float32, three steps at lr 0.05 on such gradients, is 1.5e-7 max-normalised and 4.6e-6 relative to the update.)
FP32_BASELINE = dict(adam_m=1.39e-7, adam_v=1.48e-7, adam_p_update=4.86e-6, torgb_fwd=6.84e-7, finish_dw=8.87e-8, finish_ds=8.38e-8)
FP32_FACTOR = 4.0      # -> bounds 5.6e-7, 5.9e-7, 1.9e-5, 2.7e-6, 3.5e-7, 3.4e-7


def fp32_bound(key):
    return FP32_FACTOR * FP32_BASELINE[key]


# ------------------------------------------------------------------------------------------------------------------------ optimiser
STREAM_CHUNK4 = 1024          # csrc/optim.hip:51
STREAM_MAX_BLOCKS = 256 * 16  # csrc/optim.hip:106

OPT_SIZES = [1, 3, 4, 5, 4096, 4100, 4103, 100003]
OPT_BIG = 16_777_216 + 3 * 4096 + 4 * 37 + 3       # past the cap: 4 blocks make a second round, the last chunk has 37 quads, 3 tail elements
OPT_BETAS = [(0.9, 0.999), (0.0, 0.99)]
OPT_LR, OPT_EPS = 0.05, 1e-8
SANITIZE = dict(gscale=0.5, nan=0.25, posinf=1e5, neginf=-1e5)


def optim_path(n):
    """stream_grid (csrc/optim.hip:104-109) and the chunk loop of adam_kernel / ema_kernel (:57, :89): one block per 1024-quad chunk, at most 4096
    blocks, a block strides over chunks beyond that."""
    chunks = max(1, (n // 4 + STREAM_CHUNK4 - 1) // STREAM_CHUNK4)
    return 'one_round' if chunks <= STREAM_MAX_BLOCKS else 'many_rounds'


def optim_inputs(n, seed=0):
    """p, g, m, v, p_ema as float32.  |g| spans 1e-6 .. 1e2 (log-uniform), every 7th element from the fourth on is exactly 0 (v stays 0 there;
    the sizes below 4 keep a gradient, so every case has an update to compare with)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    p = torch.randn(n, generator=gen)
    mag = torch.pow(10.0, torch.rand(n, generator=gen) * 8.0 - 6.0)
    g = mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g[3::7] = 0.0
    return dict(p=p, g=g, m=torch.zeros(n), v=torch.zeros(n), pe=torch.randn(n, generator=gen))


def nonfinite_positions(n):
    """Where the sanitising cases put NaN / +Inf / -Inf: first quad, last quad, scalar tail, and (past the cap) a chunk of the second round."""
    n4 = n // 4
    pos = []
    if n4 >= 1:
        pos += [1, (n4 - 1) * 4 + 2]
    if n % 4:
        pos += [n - 1]
    if n4 > STREAM_MAX_BLOCKS * STREAM_CHUNK4:
        pos += [STREAM_MAX_BLOCKS * STREAM_CHUNK4 * 4 + 5, n4 * 4 - 3]       # chunk 4096 (block 0, second round) and the ragged last chunk
    out = []
    for q in pos:
        if q not in out:
            out.append(q)
    return out


def poison(g):
    g = g.clone()
    vals = [float('nan'), float('inf'), -float('inf')]
    for k, q in enumerate(nonfinite_positions(g.numel())):
        g[q] = vals[k % 3]
    return g


def step_gradient(g, step):
    """The gradient of step `step`: same signs, other magnitudes (the moments then have no cancellation, so every element can be compared relatively)."""
    return g * float(step)


def as_f32(v):
    """A hyper-parameter as the kernel receives it: rounded to float32."""
    return float(torch.tensor(v, dtype=F32))


def sanitize_ref(g, scale, nan, posinf, neginf):
    """g = nan_to_num(g * scale, nan, posinf, neginf)  (include/ldetr_hip.h: ldetr_grad_sanitize_f32; csrc/optim.hip:115)."""
    g = g * scale
    g = torch.where(g != g, torch.full_like(g, nan), g)
    g = torch.where(g == math.inf, torch.full_like(g, posinf), g)
    return torch.where(g == -math.inf, torch.full_like(g, neginf), g)


def adam_ref(p, g, m, v, step, lr, beta1, beta2, eps, sanitize=None, pe=None, ema_beta=None, dtype=F64):
    """torch.optim.Adam's step without weight decay or amsgrad, the bias correction as csrc/optim.hip:40-46, :145-147 writes it:
        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    sanitize = dict(gscale, nan, posinf, neginf): g is first scaled and nan_to_num'ed.  pe: p_ema = p_new + ema_beta (p_ema - p_new).
    -> (p, m, v, pe)."""
    lr, beta1, beta2, eps = as_f32(lr), as_f32(beta1), as_f32(beta2), as_f32(eps)       # the C ABI takes them as float
    p, g, m, v = p.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype)
    if sanitize is not None:
        g = sanitize_ref(g, sanitize['gscale'], sanitize['nan'], sanitize['posinf'], sanitize['neginf'])
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    if pe is not None:
        pe = ema_ref(pe, p, ema_beta, dtype)
    return p, m, v, pe


def ema_ref(pe, p, beta, dtype=F64):
    """p_ema = p + beta (p_ema - p)  (csrc/optim.hip:155)."""
    pe, p = pe.to(dtype), p.to(dtype)
    return p + as_f32(beta) * (pe - p)


def adam_run(t, steps, betas, fuse, dtype=F64, first_step=1):
    """`steps` Adam steps from the state t (optim_inputs) with step_gradient; fuse: the gradient is poisoned and sanitised in the step.
    -> (p, m, v) in `dtype`."""
    p, m, v = t['p'], t['m'], t['v']
    for k in range(steps):
        g = step_gradient(t['g'], k + 1)
        if fuse:
            g = poison(g)
        p, m, v, _ = adam_ref(p, g, m, v, first_step + k, OPT_LR, betas[0], betas[1], OPT_EPS, SANITIZE if fuse else None, dtype=dtype)
    return p, m, v


def optim_step1000_inputs():
    """A state in the middle of training (non-zero moments) for the one case at step 1000."""
    t = optim_inputs(4103, seed=77)
    t['m'] = t['g'] * 0.5
    t['v'] = t['g'] * t['g'] * 0.7
    return t


def update_rel_err(p, p_ref, p0):
    """Error of p relative to the size of the update."""
    p, p_ref, p0 = p.detach().double().cpu(), p_ref.double(), p0.double()
    return ((p - p_ref).abs().max() / (p_ref - p0).abs().max()).item()


# ------------------------------------------------------------------------------------------------------------------------ bias_act
ACTS = ['linear', 'relu', 'lrelu', 'tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish']
ACT_INDEX = dict(linear=1, relu=2, lrelu=3, tanh=4, sigmoid=5, elu=6, selu=7, softplus=8, swish=9, gelu=10)      # csrc/bias_act.hip:33-75
HAS_2ND = {'tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish'}
BA_MAX_BLOCKS = 256 * 16      # csrc/bias_act.hip:140, :147
NT_MIN = 1 << 25              # csrc/bias_act.hip:92

# Tensors are described in storage order: `dims` are the dense dimensions as they lie in memory, `axis` the one the bias runs along (None: no bias).
# NHWC is dims (N, H, W, C) with axis 3, NCHW dims (N, C, H, W) with axis 1.
BIAS_FORMS = {
    'none': dict(dims=(3, 12, 8, 10), axis=None),
    'per_quad': dict(dims=(3, 12, 8, 10), axis=1),            # stepB = 80: one bias value per float4
    'four_consecutive': dict(dims=(3, 8, 10, 12), axis=3),    # stepB = 1, sizeB = 12
    'scalar': dict(dims=(3, 12, 5, 7), axis=1),               # stepB = 35
}


def act_defaults(act):
    return (0.0, 1.0) if act == 'gelu' else ops_ref.ACT_DEFAULTS[act]


def ba_case(name, dims, axis, act, grad, clamp=None, alpha=None, gain=None, offset=0, inplace=False, via='abi', seed=0):
    d_alpha, d_gain = act_defaults(act)
    return dict(name=name, dims=tuple(dims), axis=axis, act=act, grad=grad, clamp=clamp, alpha=float(d_alpha if alpha is None else alpha),
                gain=float(d_gain if gain is None else gain), offset=offset, inplace=inplace, via=via, seed=seed)


def bias_act_geometry(c):
    """-> (sizeX, sizeB, stepB) as torch_utils/ops/bias_act.py:42-45 hands them to the C ABI."""
    n = math.prod(c['dims'])
    if c['axis'] is None:
        return n, 0, 1
    return n, c['dims'][c['axis']], math.prod(c['dims'][c['axis'] + 1:])


def bias_act_path(c):
    """launch_bias_act (csrc/bias_act.hip:128-152): the vector kernel needs 16-byte aligned operands and sizeX % 4 == 0 and one of three bias forms,
    everything else is the scalar kernel; both cap the grid at 4096 blocks of 256 and stride beyond it; the vector kernel streams non-temporally
    when grad > 0 and sizeX >= 2^25 (:92)."""
    n, size_b, step_b = bias_act_geometry(c)
    aligned = c['offset'] % 4 == 0 and n % 4 == 0
    form = 'scalar'
    if aligned:
        if c['axis'] is None:
            form = 'none'
        elif step_b % 4 == 0:
            form = 'per_quad'
        elif step_b == 1 and size_b % 4 == 0:
            form = 'four_consecutive'
    items = n if form == 'scalar' else n // 4
    path = form + ('/stride_loop' if items > BA_MAX_BLOCKS * 256 else '/single_round')
    if form != 'scalar' and c['grad'] > 0 and n >= NT_MIN:
        path += '/non_temporal'
    return path


def _ba_cross():
    out = []
    for form, f in BIAS_FORMS.items():
        for act in ACTS:
            for grad in (0, 1, 2):
                if grad == 2 and act not in HAS_2ND:
                    continue
                out.append(ba_case(f'{form}-{act}-grad{grad}', f['dims'], f['axis'], act, grad, seed=len(out)))
    return out


BA_BIG = 4 * 4096 * 256 + 8        # quads: 2 past the capped grid's first round
BIAS_ACT_CASES = _ba_cross() + [
    ba_case('gelu-grad0-inplace', (37, 64), 1, 'gelu', 0, inplace=True, seed=200),             # training/med.py:188
    ba_case('gelu-grad0', (37, 64), 1, 'gelu', 0, seed=201),                                   # training/med.py:251
    ba_case('gelu-grad1', (37, 64), 1, 'gelu', 1, seed=202),                                   # training/med.py:262
    ba_case('gelu-grad1-scalar', (5, 7), 1, 'gelu', 1, seed=203),
    ba_case('size-not-multiple-of-4', (5, 7), 1, 'lrelu', 0, seed=204),
    ba_case('pointer-offset-one-float', (3, 12, 8, 10), 1, 'lrelu', 0, offset=1, seed=205),
    ba_case('clamp-gain-alpha-grad0', (3, 12, 8, 10), 1, 'lrelu', 0, clamp=0.9, gain=0.7, alpha=0.1, seed=206),
    ba_case('clamp-grad1', (3, 12, 8, 10), 1, 'lrelu', 1, clamp=0.9, seed=207),
    ba_case('clamp-grad2', (3, 8, 10, 12), 3, 'tanh', 2, clamp=0.9, gain=1.3, seed=208),
    ba_case('wrapper-dim0', (12, 6, 8), 0, 'lrelu', 1, via='wrapper', seed=209),
    ba_case('wrapper-dim2', (12, 6, 8), 2, 'lrelu', 1, via='wrapper', seed=210),
    ba_case('wrapper-clamp-backward', (3, 12, 8, 10), 1, 'lrelu', 1, clamp=0.9, via='wrapper', seed=211),
    ba_case('past-grid-cap-none', (BA_BIG,), None, 'lrelu', 0, seed=212),
    ba_case('past-grid-cap-per-quad', (BA_BIG // 8, 8), 0, 'lrelu', 0, seed=213),
    ba_case('past-grid-cap-four-consecutive', (BA_BIG // 8, 8), 1, 'lrelu', 0, seed=214),
    ba_case('past-grid-cap-scalar', (149797, 7), 1, 'lrelu', 0, seed=215),                      # 1,048,579 elements > 4096 x 256
    # the lrelu backward of the 256 x 256 x 32 synthesis layer at 16 samples, channels-last, with a bias: exactly 2^25 elements
    ba_case('bench-lrelu-grad1-2^25', (16, 256, 256, 32), 3, 'lrelu', 1, seed=216),
]
BIAS_ACT_PATHS = [f'{form}/{rounds}' for form in BIAS_FORMS for rounds in ('single_round', 'stride_loop')] + ['four_consecutive/stride_loop/non_temporal']


def bias_act_inputs(c):
    """-> x, b, dy, ddx (float32, storage order).  grad 0 uses x and b; grad 1 also the incoming gradient dy; grad 2 also ddx, the incoming
    gradient of the first gradient."""
    gen = torch.Generator().manual_seed(5000 + c['seed'])
    dims = c['dims']
    x = torch.randn(dims, generator=gen) * 2
    b = torch.randn(dims[c['axis']], generator=gen) if c['axis'] is not None else None
    dy = torch.randn(dims, generator=gen)
    ddx = torch.randn(dims, generator=gen)
    return x, b, dy, ddx


def _gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0))))      # csrc/bias_act.hip:72-75


def bias_act_ref(x, b, axis, act, alpha, gain, clamp, dy=None, ddx=None, dtype=F64):
    """-> (y, dx, d_x): y = clamp(act(x + b) * gain); dx = dy * dy/dx (grad 1, when dy is given); d_x = the gradient of <ddx, dx> with respect to
    x (grad 2, when ddx is given too), all by autograd in `dtype`."""
    x = x.to(dtype).clone().requires_grad_(True)
    b = b.to(dtype) if b is not None else None
    if act == 'gelu':
        shape = [1] * x.ndim
        if b is not None:
            shape[axis] = -1
        y = _gelu(x + b.reshape(shape) if b is not None else x) * gain
        if clamp is not None and clamp >= 0:
            y = y.clamp(-clamp, clamp)
    else:
        y = ops_ref.bias_act(x, b, dim=axis if axis is not None else 1, act=act, alpha=alpha, gain=gain, clamp=clamp)
    dx = d_x = None
    if dy is not None:
        (dx,) = torch.autograd.grad(y, x, dy.to(dtype), create_graph=ddx is not None)
        if ddx is not None:
            if dx.requires_grad:
                (d_x,) = torch.autograd.grad(dx, x, ddx.to(dtype), allow_unused=True)
            d_x = torch.zeros_like(x) if d_x is None else d_x
    return y.detach(), (dx.detach() if dx is not None else None), (d_x.detach() if d_x is not None else None)


# ------------------------------------------------------------------------------------------------------------------------ toRGB
def torgb_inputs(B, P, C, seed=0):
    gen = torch.Generator().manual_seed(9000 + seed + 7 * B + P + C)
    r = lambda *s: torch.randn(*s, generator=gen)
    return dict(x=r(B, P, C), w=r(3, C) / math.sqrt(C), s=r(B, C) * 0.5 + 1.0, bias=r(3) * 0.1, dy=r(B, P, 3), dw0=r(3, C))


def torgb_fwd_ref(x, w, s, bias=None, dtype=F64):
    """y[b][p][o] = bias[o] + sum_c x[b][p][c] w[o][c] s[b][c]  (include/ldetr_hip.h: ldetr_torgb_fwd_f32)."""
    y = torch.einsum('bpc,oc,bc->bpo', x.to(dtype), w.to(dtype), s.to(dtype))
    return y + bias.to(dtype) if bias is not None else y


def torgb_bwd_ref(x, dy, w, s, dtype=F64):
    """dx = s * (dy @ w);  dws[b] = dy[b]^T x[b];  dbias = dy.sum((0, 1))  (csrc/misc_ops.hip:266-269)."""
    x, dy, w, s = x.to(dtype), dy.to(dtype), w.to(dtype), s.to(dtype)
    dx = s[:, None, :] * (dy @ w)
    dws = dy.transpose(1, 2) @ x
    return dx, dws, dy.sum((0, 1))


def torgb_finish_ref(dws, s, w, dw0, dtype=F64):
    """dw = dw0 + sum_b dws[b] * s[b];  ds[b] = sum_o dws[b, o] * w[o]  (csrc/misc_ops.hip:341-343)."""
    dws, s, w = dws.to(dtype), s.to(dtype), w.to(dtype)
    return dw0.to(dtype) + (dws * s[:, None, :]).sum(0), (dws * w[None]).sum(1)


TORGB_FWD_MAX_GX = 4096       # csrc/misc_ops.hip:691


def torgb_fwd_path(B, P, C, styles_stride=None):
    """hip/modconv.py:143 sends what ldetr_torgb_fwd_f32 cannot take to the contraction engine; the kernel is instantiated for lpp = min(C / 4, 64)
    lanes per pixel (csrc/misc_ops.hip:689, :694-702), makes C / 4 / lpp trips (:645, :661) and caps grid.x at 4096 blocks of 256 / lpp pixels (:690-691)."""
    c4 = C // 4
    if C % 4 or C > 512 or c4 < 1 or c4 & (c4 - 1) or (styles_stride is not None and styles_stride != C):
        return 'engine_fallback'
    lpp = min(c4, 64)
    ppb = 256 // lpp
    capped = (P + ppb - 1) // ppb > TORGB_FWD_MAX_GX
    return f'lpp{lpp}/trips{c4 // lpp}/' + ('grid_capped' if capped else 'grid_under_cap')


def torgb_bwd_path(B, P, C):
    """ldetr_torgb_bwd_f32 (csrc/misc_ops.hip:713-718) and torgb_bwd_kernel (:279-284): TQ = min(C / 4, 256) quads across, RL = 256 / TQ row lanes
    (256 - TQ RL threads idle), 16 RL rows per block doubled while there are more than 2048 blocks, grid.z = ceil(C / 4 / TQ)."""
    c4 = C // 4
    tq = min(c4, 256)
    rl = 256 // tq
    gz = (c4 + tq - 1) // tq
    rows = rl * 16
    doubled = False
    while ((P + rows - 1) // rows) * B * gz > 2048:
        rows *= 2
        doubled = True
    return f'RL{rl}' + ('/idle_threads' if rl * tq < 256 else '') + f'/gz{gz}' + ('/rows_doubled' if doubled else '')


# (B, P, C, how): 'abi' = ldetr_torgb_fwd_f32, 'abi_nobias' = bias NULL, 'wrapper' = hip.modconv.torgb_fwd, 'wrapper_strided' = styles a view
# whose rows are further apart than C
TORGB_FWD_CASES = [(3, 37, C, 'abi') for C in (4, 8, 16, 32, 64, 128, 256, 512)] + [
    (1, 1, 4, 'abi'), (1, 1, 512, 'abi'), (3, 37, 32, 'abi_nobias'), (3, 37, 512, 'abi_nobias'), (1, 16384 + 3, 256, 'abi'),
    (3, 37, 512, 'wrapper'), (3, 37, 96, 'wrapper'), (2, 37, 1024, 'wrapper'), (3, 37, 64, 'wrapper_strided')]
TORGB_FWD_PATHS = [f'lpp{l}/trips1/grid_under_cap' for l in (1, 2, 4, 8, 16, 32, 64)] + ['lpp64/trips2/grid_under_cap', 'lpp64/trips1/grid_capped', 'engine_fallback']


def torgb_fwd_case_path(case):
    B, P, C, how = case
    return torgb_fwd_path(B, P, C, styles_stride=C + 4 if how == 'wrapper_strided' else None)


TORGB_BWD_CASES = [(B, P, C) for C in (4, 32, 96, 512, 1028) for (B, P) in ((3, 37), (1, 1))] + [(1, 16 * 1025 + 3, 1028)]
TORGB_BWD_PATHS = ['RL256/gz1', 'RL32/gz1', 'RL10/idle_threads/gz1', 'RL2/gz1', 'RL1/gz2', 'RL1/gz2/rows_doubled']
# finish kernel: one thread per element of dw (3C) and of ds (B C) in a grid of max(B, 3) C threads; the two ranges end in different blocks
TORGB_FINISH_CASES = [(1, 100), (2, 100), (5, 60), (3, 512), (1, 4)]


def finish_inputs(B, C):
    gen = torch.Generator().manual_seed(9500 + 31 * B + C)
    r = lambda *s: torch.randn(*s, generator=gen)
    return dict(dws=r(B, 3, C) * 4.0, s=r(B, C) * 0.5 + 1.0, w=r(3, C) / math.sqrt(C), dw0=r(3, C))


def finish_last_blocks(B, C):
    """-> (block of the last dw element, block of the last ds element, blocks launched)  (csrc/misc_ops.hip:347-354, :750-751)."""
    return (3 * C - 1) // 256, (B * C - 1) // 256, (max(B, 3) * C + 255) // 256


# ------------------------------------------------------------------------------------------------------------------------ max-pool
POOL_MAX_BLOCKS = 8192        # csrc/misc_ops.hip:610, :622


def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def maxpool_path(N, H, W, C, direction):
    """One thread per channel quad of the output (forward) or the input (backward), grid capped at 8192 blocks of 256 with a stride loop beyond."""
    total = N * (pool_out(H) * pool_out(W) if direction == 'fwd' else H * W) * (C // 4)
    return f'{direction}/' + ('stride_loop' if total > POOL_MAX_BLOCKS * 256 else 'single_round')


POOL_SHAPES = [(1, 1), (1, 7), (2, 2), (13, 12), (12, 13), (64, 64)]
POOL_CHANNELS = [4, 8, 64]
POOL_KINDS = ['signed', 'negative', 'ties', 'nonfinite', 'all_neg_inf']
POOL_CASES = [(2, H, W, C, kind) for (H, W) in POOL_SHAPES for C in POOL_CHANNELS for kind in POOL_KINDS if kind in ('signed', 'ties') or C == 8]
POOL_BIG_BWD = (1, 364, 364, 64, 'signed')
POOL_BIG_FWD = (1, 363, 363, 256, 'signed')
POOL_PATHS = ['fwd/single_round', 'fwd/stride_loop', 'bwd/single_round', 'bwd/stride_loop']


def pool_inputs(N, H, W, C, kind, seed=0):
    """-> x [N, C, H, W] float32 and dy [N, C, OH, OW] (multiples of 1/8: the up to four gradients an input element collects add exactly)."""
    gen = torch.Generator().manual_seed(7000 + seed + 13 * H + W + C)
    x = torch.randn(N, C, H, W, generator=gen)
    if kind == 'negative':
        x = -x.abs() - 0.5
    elif kind == 'ties':
        x = (x * 2).round() / 2
    elif kind == 'all_neg_inf':
        x[0] = -math.inf
    elif kind == 'nonfinite':
        flat = x.view(-1)
        n = flat.numel()
        flat[n // 3] = math.nan
        flat[min(n - 1, n // 2 + 1)] = math.inf
        flat[n - 1 - n // 5] = -math.inf
    dy = (torch.randn(N, C, pool_out(H), pool_out(W), generator=gen) * 8).round() / 8
    return x, dy


def maxpool_ref(x, dy):
    """F.max_pool2d(x.double(), 3, 2, 1) and its autograd -> (y, dx), NCHW float64."""
    xr = x.double().clone().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    (dx,) = torch.autograd.grad(y, xr, dy.double())
    return y.detach(), dx


def equal_with_nan(a, b):
    """Bit-for-bit after the cast, NaN positions compared separately."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    na, nb = a != a, b != b
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na], b[~nb]))


# ------------------------------------------------------------------------------------------------------------------------ float32 yardstick
def measure_fp32_baselines(include_big=False):
    """The float32 CPU evaluation of every formula that has no project bound against its float64 evaluation, worst case over the tables
    (include_big: with the past-the-cap optimiser case, as the recorded figures were taken) -> dict like FP32_BASELINE."""
    out = dict.fromkeys(FP32_BASELINE, 0.0)

    def adam(t, steps, betas, fuse, first_step=1):
        p64, m64, v64 = adam_run(t, steps, betas, fuse, F64, first_step)
        p32, m32, v32 = adam_run(t, steps, betas, fuse, F32, first_step)
        out['adam_m'] = max(out['adam_m'], elem_rel_err(m32, m64))
        out['adam_v'] = max(out['adam_v'], elem_rel_err(v32, v64))
        out['adam_p_update'] = max(out['adam_p_update'], update_rel_err(p32, p64, t['p']))
    for n in OPT_SIZES:
        for betas in OPT_BETAS:
            for fuse in (0, 1):
                adam(optim_inputs(n, seed=n), 3, betas, fuse)
    adam(optim_step1000_inputs(), 1, OPT_BETAS[0], 0, first_step=1000)
    if include_big:
        adam(optim_inputs(OPT_BIG, seed=1), 1, OPT_BETAS[0], 1)
    for B, P, C, how in TORGB_FWD_CASES:
        t = torgb_inputs(B, P, C)
        bias = None if how == 'abi_nobias' else t['bias']
        out['torgb_fwd'] = max(out['torgb_fwd'], rel_err(torgb_fwd_ref(t['x'], t['w'], t['s'], bias, F32), torgb_fwd_ref(t['x'], t['w'], t['s'], bias)))
    for B, C in TORGB_FINISH_CASES:
        t = finish_inputs(B, C)
        dw64, ds64 = torgb_finish_ref(t['dws'], t['s'], t['w'], t['dw0'])
        dw32, ds32 = torgb_finish_ref(t['dws'], t['s'], t['w'], t['dw0'], F32)
        out['finish_dw'] = max(out['finish_dw'], rel_err(dw32, dw64))
        out['finish_ds'] = max(out['finish_ds'], rel_err(ds32, ds64))
    return out
