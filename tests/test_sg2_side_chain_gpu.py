"""The grouped launches of the StyleGAN2 side chain, kernel level: ldetr_gemm_small_group_f32 (csrc/gemm_conv.hip), ldetr_demod_group_fwd/bwd_f32
(csrc/demod.hip), ldetr_sg2_affine_bwd_f32 (csrc/sg2_affine.hip) and ldetr_torgb_fwd_add_f32 (csrc/misc_ops.hip).

The forward kernels run the device bodies of the single launches, so they are held to bit equality with those.  The backward kernels are held to
the formulas of include/ldetr_hip.h in float64 at 4 x the float32 yardstick -- the same formulas evaluated by torch in float32 on the host, measured
here against float64 (the rule of tests/token_stack_common.py) -- and, for inputs whose sums are exact in any order, to equality."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
NAN_BITS = 0x7FC01234


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def guarded(rows, cols, dev, rows_guard=2):
    """-> (buffer with NaN-filled guard rows in front of and behind a [rows, cols] view, the view)."""
    buf = torch.full((rows + 2 * rows_guard, cols), float('nan'), device=dev, dtype=F32)
    buf.view(torch.int32).fill_(NAN_BITS)
    return buf, buf[rows_guard:rows_guard + rows]


def guards_intact(buf, rows, rows_guard=2):
    bits = buf.view(torch.int32)
    return bool((bits[:rows_guard] == NAN_BITS).all()) and bool((bits[rows_guard + rows:] == NAN_BITS).all())


# ------------------------------------------------------------------------------------------------------------------------------ grouped GEMM
def _gemm_case(dev, M, K, Ns, seed, posts=None):
    from layoutdetr_amd.hip import core
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dev)
    ws = [(torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev) for N in Ns]
    bs = [torch.randn(N, generator=g).to(dev) for N in Ns]
    alone = [core.gemm(x, w, 0, 0, M, N, K, ep=core.epilogue(alpha=0.37, col_bias=b)) for w, b, N in zip(ws, bs, Ns)]
    if posts is not None:
        alone = [a * float(p) for a, p in zip(alone, posts)]
    bufs, outs = zip(*[guarded(M, N, dev) for N in Ns])
    problems = [dict(A=x, B=w, M=M, N=N, K=K, out=o, ep=core.epilogue(alpha=0.37, col_bias=b)) for w, b, N, o in zip(ws, bs, Ns, outs)]
    return problems, alone, bufs, outs


@pytest.mark.parametrize('Ns', [(32, 64, 96), (64,)])
@pytest.mark.parametrize('posts', [None, 'scaled'])
def test_grouped_gemm_equals_single_launches(dev, Ns, posts):
    """M = 3, K = 32: three problems of 1, 2 and 3 column tiles, and a table of one; with and without the post factor (a separate torch mul)."""
    from layoutdetr_amd.hip import core
    ps = None if posts is None else [1.0 / math.sqrt(n) for n in Ns]
    problems, alone, bufs, outs = _gemm_case(dev, 3, 32, Ns, 5, ps)
    assert core.gemm_group(problems, ps)
    assert core.launched_kernel('gemm').startswith('gemm_small_group_kernel<4w')
    torch.cuda.synchronize()
    for o, a, buf in zip(outs, alone, bufs):
        assert torch.equal(o, a)
        assert guards_intact(buf, 3)


def test_grouped_gemm_eight_wave_instantiation(dev):
    """M = 16, K = 512, N in {32, 512}: the shapes of the 256^2 network's affines, the 8-wave instantiation with scalar-addressed loads."""
    from layoutdetr_amd.hip import core
    ps = [1.0, 1.0 / math.sqrt(512)]
    problems, alone, bufs, outs = _gemm_case(dev, 16, 512, (32, 512), 6, ps)
    assert core.gemm_group(problems, ps)
    assert core.launched_kernel('gemm') == 'gemm_small_group_kernel<8w,FAST>'
    torch.cuda.synchronize()
    for o, a, buf in zip(outs, alone, bufs):
        assert torch.equal(o, a)
        assert guards_intact(buf, 16)


def test_grouped_gemm_refuses_mixed_instantiations(dev):
    """K = 32 takes 4 waves, K = 512 on one tile takes 8: no common instantiation, the entry returns the unsupported code and launches nothing."""
    from layoutdetr_amd import _lib
    from layoutdetr_amd.hip import core
    p4, _, _, o4 = _gemm_case(dev, 3, 32, (32,), 7)
    p8, _, _, o8 = _gemm_case(dev, 16, 512, (32,), 8)
    before = core.engine_launch_counts()
    assert core.gemm_group(p4 + p8) is False
    assert core.engine_launch_counts() == before
    assert b'another instantiation' in _lib.load().ldetr_last_error()
    torch.cuda.synchronize()
    assert bool(o4[0].isnan().all()) and bool(o8[0].isnan().all())


# ------------------------------------------------------------------------------------------------------------------------------ grouped demod
DEMOD_LAYERS = [(8, 8, 3), (64, 32, 3), (32, 64, 3), (32, 16, 1)]      # (O, I, taps): 3x3 layers and one 1x1
DB = 3


@pytest.fixture(scope='module')
def demod_case(dev):
    """Weights (channels_last parameters, as SynthesisLayer holds them), styles, upstream gradients; the grouped forward's outputs; the
    float64 references and the float32 yardsticks of the backward, computed once and left unchanged."""
    from layoutdetr_amd.hip import sg2_chain
    g = torch.Generator().manual_seed(21)
    ws = [(torch.randn(O, I, k, k, generator=g) / math.sqrt(I * k * k)) for O, I, k in DEMOD_LAYERS]
    ss = [torch.randn(DB, I, generator=g) * 0.5 + 1.0 for O, I, k in DEMOD_LAYERS]
    gs = [torch.randn(DB, O, generator=g) for O, I, k in DEMOD_LAYERS]
    dw0 = [torch.randn(O, I, k, k, generator=g) for O, I, k in DEMOD_LAYERS]
    ds0 = [torch.randn(DB, I, generator=g) for O, I, k in DEMOD_LAYERS]
    wd = [w.to(dev).contiguous(memory_format=torch.channels_last) for w in ws]
    sd = [s.to(dev) for s in ss]
    d, w2 = sg2_chain.side_demod(wd, sd)

    def formulas(dt):
        out = []
        for w, s, gg, a, b in zip(ws, ss, gs, dw0, ds0):
            w, s, gg = w.to(dt), s.to(dt), gg.to(dt)
            W2 = w.square().sum(dim=[2, 3])
            dc = (s.square() @ W2.t() + 1e-8).rsqrt()
            t = -0.5 * gg * dc ** 3
            dw = a.to(dt) + 2 * w * (t.t() @ s.square())[:, :, None, None]
            ds = b.to(dt) + 2 * s * (t @ W2)
            out.append((dw, ds))
        return out
    return dict(ws=wd, ss=sd, gs=[t.to(dev) for t in gs], dw0=dw0, ds0=ds0, d=d, w2=w2, ref=formulas(F64), yard=formulas(F32))


def test_grouped_demod_forward_equals_single_launches(dev, demod_case):
    from layoutdetr_amd.hip import core
    c = demod_case
    for (O, I, k), w, s, d, w2 in zip(DEMOD_LAYERS, c['ws'], c['ss'], c['d'], c['w2']):
        d1 = torch.empty((DB, O), device=dev); w21 = torch.empty((O, I), device=dev)
        st = w.stride()
        core.check(core.lib().ldetr_demod_fwd_f32(core.ptr(w), st[0], st[1], st[2], st[3], core.ptr(s), core.ptr(d1), core.ptr(w21), DB, O, I, k, k, 1e-8,
                                                  core.stream()), 'demod_fwd')
        assert torch.equal(d, d1) and torch.equal(w2, w21), (O, I, k)


def test_grouped_demod_backward_accumulates_within_four_yardsticks(dev, demod_case):
    """dw accumulated onto a pre-filled buffer (the weight's strides), ds added onto a pre-filled ds, against the header's formulas in float64."""
    from layoutdetr_amd.hip import sg2_chain
    c = demod_case
    dws = [a.to(dev).contiguous(memory_format=torch.channels_last) for a in c['dw0']]
    dss = [b.to(dev).clone() for b in c['ds0']]
    layers = list(zip(c['ws'], c['ss'], c['d'], c['w2']))
    sg2_chain.side_demod_bwd(layers, list(zip(c['gs'], dws, dss)), DB)
    torch.cuda.synchronize()
    for L, dw, ds, (dw64, ds64), (dw32, ds32) in zip(DEMOD_LAYERS, dws, dss, c['ref'], c['yard']):
        for name, got, r64, r32 in (('dw', dw, dw64, dw32), ('ds', ds, ds64, ds32)):
            yard = rel(r32, r64)
            err = rel(got, r64)
            print(f'demod_group_bwd {L} {name}: err {err:.3e} yardstick {yard:.3e}')
            assert err <= 4 * yard, (L, name, err, yard)


def test_grouped_demod_backward_skips_a_null_weight_gradient(dev, demod_case):
    """dweight NULL (a frozen conv weight): the style gradient alone, added onto zeros.  1e-5: sums of at most 64 fp32 terms of one sign pattern,
    64 x 2^-24 = 4e-6 in the worst case."""
    from layoutdetr_amd.hip import sg2_chain
    c = demod_case
    dss = [torch.zeros_like(b).to(dev) for b in c['ds0']]
    layers = list(zip(c['ws'], c['ss'], c['d'], c['w2']))
    sg2_chain.side_demod_bwd(layers, [(g, None, ds) for g, ds in zip(c['gs'], dss)], DB)
    torch.cuda.synchronize()
    for ds, b, (_, ds64) in zip(dss, c['ds0'], c['ref']):
        assert rel(ds, ds64 - b.double()) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------------------ affine backward
def _affine_inputs(kind, Cs, B, D, seed):
    g = torch.Generator().manual_seed(seed)

    def draw(shape, std=1.0):
        if kind == 'dyadic':      # small integers / quarters: every partial sum is a float32, the order of summation does not matter
            return torch.randint(-4, 5, shape, generator=g).float() / 4
        return torch.randn(shape, generator=g) * std
    t = dict(ws=draw((B, D)), ds=[draw((B, C)) for C in Cs], A=[draw((C, D), 1.0 / math.sqrt(D)) for C in Cs],
             dA0=[draw((C, D)) for C in Cs], db0=[draw((C,)) for C in Cs])
    t['gain'] = [0.25 if kind == 'dyadic' else 1.0 / math.sqrt(D)] * len(Cs)
    t['post'] = [(0.5 if kind == 'dyadic' else 1.0 / math.sqrt(C)) if i % 2 else 1.0 for i, C in enumerate(Cs)]
    return t


def _affine_formulas(t, dt):
    dws = torch.zeros_like(t['ws'], dtype=dt)
    dA, db = [], []
    for ds, A, a0, b0, gain, post in zip(t['ds'], t['A'], t['dA0'], t['db0'], t['gain'], t['post']):
        ds, A = ds.to(dt), A.to(dt)
        scale = float(torch.tensor(gain * post, dtype=F32))       # the c_float the descriptor holds
        dws = dws + scale * (ds @ A)
        dA.append(a0.to(dt) + scale * (ds.t() @ t['ws'].to(dt)))
        db.append(b0.to(dt) + float(torch.tensor(post, dtype=F32)) * ds.sum(0))
    return dws, dA, db


AFFINE_TABLES = [((32,), 3, 32), ((8, 32, 64, 64, 32), 3, 32), ((64, 8), 5, 96)]     # (Cin per layer, B, w_dim); 96: two column groups, the second one half full


@pytest.mark.parametrize('Cs,B,D', AFFINE_TABLES)
@pytest.mark.parametrize('kind', ['dyadic', 'gauss'])
def test_affine_backward(dev, Cs, B, D, kind):
    """Tables of 1 and of 5 layers with Cin in {8, 32, 64}; gradients accumulated onto pre-filled targets.  'dyadic': equality with float64;
    'gauss': 4 x the float32 yardstick."""
    from layoutdetr_amd.hip import sg2_chain
    t = _affine_inputs(kind, Cs, B, D, 40 + len(Cs))
    ref, yard = _affine_formulas(t, F64), _affine_formulas(t, F32)
    dA = [a.to(dev).clone() for a in t['dA0']]
    db = [b.to(dev).clone() for b in t['db0']]
    layers = [(ds.to(dev), A.to(dev), a, b, gain, post) for ds, A, a, b, gain, post in zip(t['ds'], t['A'], dA, db, t['gain'], t['post'])]
    dws = sg2_chain.side_affine_bwd(t['ws'].to(dev), layers)
    torch.cuda.synchronize()
    got = [('dws', dws, ref[0], yard[0])] + [(f'dA{i}', a, r, y) for i, (a, r, y) in enumerate(zip(dA, ref[1], yard[1]))] \
        + [(f'db{i}', b, r, y) for i, (b, r, y) in enumerate(zip(db, ref[2], yard[2]))]
    for name, g_, r64, r32 in got:
        if kind == 'dyadic':
            assert torch.equal(g_.double().cpu(), r64), name
        else:
            y, e = rel(r32, r64), rel(g_, r64)
            print(f'affine_bwd {Cs} {name}: err {e:.3e} yardstick {y:.3e}')
            assert e <= 4 * y, (name, e, y)


def test_affine_backward_without_parameter_gradients(dev):
    """dA and db NULL (frozen affines): the latent's gradient alone."""
    from layoutdetr_amd.hip import sg2_chain
    t = _affine_inputs('dyadic', (32, 8), 3, 32, 50)
    layers = [(ds.to(dev), A.to(dev), None, None, gain, post) for ds, A, gain, post in zip(t['ds'], t['A'], t['gain'], t['post'])]
    dws = sg2_chain.side_affine_bwd(t['ws'].to(dev), layers)
    assert torch.equal(dws.double().cpu(), _affine_formulas(t, F64)[0])


# ------------------------------------------------------------------------------------------------------------------------------ toRGB + addend
@pytest.mark.parametrize('R', [4, 8])
def test_torgb_with_addend_equals_kernel_plus_add(dev, R):
    from layoutdetr_amd.hip import core, modconv, sg2_chain
    g = torch.Generator().manual_seed(60 + R)
    B, C = 3, 64
    x = torch.randn(B, R, R, C, generator=g).to(dev); w = torch.randn(3, C, generator=g).to(dev)
    s = torch.randn(B, C, generator=g).to(dev); b = torch.randn(3, generator=g).to(dev)
    img = torch.randn(B, R, R, 3, generator=g).to(dev)
    want = img + modconv.torgb_fwd(x, w, s, b)
    got = sg2_chain._torgb_fwd(x, w, s, b, img)
    assert torch.equal(got, want)
    assert torch.equal(sg2_chain._torgb_fwd(x, w, s, b, None), modconv.torgb_fwd(x, w, s, b))
