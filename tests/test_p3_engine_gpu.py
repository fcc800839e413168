"""Path-complete parity of the plane-format conv engine (csrc/p3_engine.hip) through the C ABI, against the float64 references of
tests/p3_engine_common.py.  tests/test_p3_engine_ref_cpu.py proves the tables, the references, the preconditions and the bars without a GPU.

For every table case, in every input class that applies: the ten fields of ldetr_p3_last_launch equal the policy model's (which makes the path list
true), the values meet the class's bar (bit equality for select / select_w / grid, FP32_FACTOR x the float32 yardstick in two measures for rounding),
every output sits between sentinel bands that must come back untouched, a P3 output merges to the fp32 output bit for bit, and a split-K launch
repeated gives the same bits (a counter that was not re-armed or a shared slot would change them)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import p3_engine_common as P

pytestmark = pytest.mark.gpu
P.limit_threads()
F64, F32 = P.F64, P.F32
GUARD = 4096                                                    # sentinel bytes on either side of every output
SWEEP_FORCED = 'P3_' in os.environ.get('LDETR_DEBUG', '')      # a development sweep is forcing tiles / split-K / pairing: the model describes the default policy
KEYS = ('kind', 'bm', 'bn', 'nw', 'splitk', 'xm', 'xn', 'ncls', 'tn_splitk', 'grid')
WORST = {}                                                      # (family, K bucket, measure) -> worst figure seen, printed by the last test


@pytest.fixture(scope='module')
def L(dev):
    from layoutdetr_amd.hip import core
    return core.lib()


def _core():
    from layoutdetr_amd.hip import core
    return core


def last_launch(L):
    info = (ctypes.c_int32 * 10)()
    _core().check(L.ldetr_p3_last_launch(info), 'last_launch')
    return dict(zip(KEYS, list(info)))


def p3_split(L, x2d):
    core = _core()
    rows, C = x2d.shape
    out = torch.empty(rows * C * 6, dtype=torch.uint8, device=x2d.device)
    core.check(L.ldetr_p3_split_f32(core.ptr(x2d), x2d.stride(0), core.ptr(out), rows, C, core.stream()), 'split')
    return out


def p3_merge(L, p, rows, C):
    core = _core()
    out = torch.empty(rows, C, dtype=torch.float32, device=p.device)
    core.check(L.ldetr_p3_merge_f32(core.ptr(p), core.ptr(out), C, rows, C, core.stream()), 'merge')
    return out


def p3_of(L, dev, t):
    """fp32 CPU tensor [..., C] -> its P3 image on the device."""
    return p3_split(L, t.to(dev).reshape(-1, t.shape[-1]).contiguous())


class Guarded:
    """nbytes of output between two sentinel bands; the inside starts as 0xFF bytes (NaN as fp32: an element the kernel leaves out shows)."""

    def __init__(self, dev, nbytes, init=None):
        self.n = nbytes
        self.buf = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=dev)
        self.pattern = ((torch.arange(GUARD, device=dev) * 7 + 13) % 251).to(torch.uint8)
        self.buf[:GUARD] = self.pattern
        self.buf[GUARD + nbytes:] = self.pattern
        self.inner = self.buf[GUARD:GUARD + nbytes]
        self.inner.fill_(0xFF)
        if init is not None:
            self.f32().copy_(init.reshape(-1))

    def f32(self):
        return self.inner.view(torch.float32)

    def ptr(self):
        return ctypes.c_void_p(self.inner.data_ptr())

    def check(self, what):
        assert torch.equal(self.buf[:GUARD], self.pattern), what + ': bytes BEFORE the output were written'
        assert torch.equal(self.buf[GUARD + self.n:], self.pattern), what + ': bytes AFTER the output were written'


def same_bits(a, b):
    """fp32 tensors equal element for element; NaN by position, -0 == +0."""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def make_epilogue(L, dev, t, e, keep):
    """-> ldetr_p3_epilogue of the case's operands (device tensors are parked in `keep`)."""
    from layoutdetr_amd import _lib
    ep = _lib.P3Epilogue()
    ep.alpha = float(t.get('alpha', 1.0))
    for field, key in (('col_scale', 'scale'), ('col_bias', 'bias'), ('residual_f32', 'res_f32')):
        if e[key]:
            d = t[key].to(dev).contiguous(); keep.append(d)
            setattr(ep, field, d.data_ptr())
    if e['res_p3']:
        d = p3_of(L, dev, t['res_p3']); keep.append(d); ep.residual_p3 = d.data_ptr()
    if e['mask']:
        d = p3_of(L, dev, t['mask']); keep.append(d); ep.relu_mask_p3 = d.data_ptr()
    ep.relu = 1 if e['relu'] else 0
    return ep


class Out:
    """The fp32 and / or P3 output of one launch, each between sentinels."""

    def __init__(self, L, dev, rows, C, store):
        self.L, self.rows, self.C = L, rows, C
        self.f = Guarded(dev, rows * C * 4) if store in ('f32', 'both') else None
        self.p = Guarded(dev, rows * C * 6) if store in ('p3', 'both') else None

    def ptrs(self):
        return (self.p.ptr() if self.p else None, self.f.ptr() if self.f else None)

    def value(self, what):
        """Checks the footprint and the P3-store equality -> the fp32 output [rows, C] (merged from P3 when that is the only store)."""
        torch.cuda.synchronize()
        for g in (self.f, self.p):
            if g is not None:
                g.check(what)
        merged = p3_merge(self.L, self.p.inner, self.rows, self.C) if self.p else None
        if self.f is None:
            return merged
        v = self.f.f32().reshape(self.rows, self.C).clone()
        if merged is not None:
            assert same_bits(merged, v), what + ': merge(out_p3) is not the fp32 output'
        return v


class Workspace:
    """ws=False: the split-K workspace is unregistered for the launches inside, and registered again whatever happens."""

    def __init__(self, L, on):
        self.L, self.on = L, on

    def __enter__(self):
        if not self.on:
            _core().check(self.L.ldetr_set_workspace(None, 0), 'unregister')

    def __exit__(self, *a):
        if not self.on:
            ws = _core()._workspace[torch.cuda.current_device()]
            _core().check(self.L.ldetr_set_workspace(ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4), 're-register')


def rewind(L):
    """Registers the split-K workspace again, which rewinds its counter and partial-tile rings (csrc/gemm_conv.hip: ldetr_set_workspace): the next
    split-K launch takes the counters and slots at the START of the rings.  A launch, a rewind and the same launch again therefore meet the counters the
    first one left behind -- they must be zero again -- where two launches in a row would each get a fresh stretch of the ring."""
    ws = _core()._workspace[torch.cuda.current_device()]
    _core().check(L.ldetr_set_workspace(ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4), 'rewind')


# ------------------------------------------------------------------------------------------------------------------------ launches
def launch_fwd(L, dev, c, ts, keep):
    """ts: one input dict (fwd) or two (dual) -> ([fp32 outputs], launch record)"""
    core = _core()
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    OH, OW = P.out_hw(H, W, KH, KW, s, pad)
    es = [c['epi'], c['epi2']][:len(ts)]
    xs = [p3_of(L, dev, t['x']) for t in ts]
    ws = [p3_of(L, dev, t['w'].reshape(Co, -1)) for t in ts]
    eps = [make_epilogue(L, dev, t, e, keep) for t, e in zip(ts, es)]
    outs = [Out(L, dev, N * OH * OW, Co, e['store']) for e in es]
    with Workspace(L, c['ws']):
        if len(ts) == 1:
            core.check(L.ldetr_p3_conv2d_fwd(core.ptr(xs[0]), N, H, W, Ci, core.ptr(ws[0]), Co, KH, KW, s, pad, ctypes.byref(eps[0]), *outs[0].ptrs(), core.stream()), 'fwd')
        else:
            core.check(L.ldetr_p3_conv2d_fwd_dual(core.ptr(xs[0]), core.ptr(xs[1]), N, H, W, Ci, core.ptr(ws[0]), core.ptr(ws[1]), Co, KH, KW, s, pad,
                                                  ctypes.byref(eps[0]), ctypes.byref(eps[1]), *outs[0].ptrs(), *outs[1].ptrs(), core.stream()), 'fwd_dual')
        rec = last_launch(L)
        vals = [o.value(c['name']).reshape(N, OH, OW, Co) for o in outs]
    return vals, rec


def _weight_bwd(L, dev, c, t):
    core = _core()
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    w = t['w'].to(dev).contiguous()
    sc = t['row_scale'].to(dev) if c['row_scale'] else None
    wb = torch.empty(Ci * KH * KW * Co * 6, dtype=torch.uint8, device=dev)
    core.check(L.ldetr_p3_weight_bwd(core.ptr(w), core.ptr(sc), core.ptr(wb), Co, KH, KW, Ci, core.stream()), 'weight_bwd')
    return wb


def launch_dgrad(L, dev, c, t, keep):
    core = _core()
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    OH, OW = P.out_hw(H, W, KH, KW, s, pad)
    dyp, wb = p3_of(L, dev, t['dy']), _weight_bwd(L, dev, c, t)
    ep = make_epilogue(L, dev, t, c['epi'], keep)
    out = Out(L, dev, N * H * W, Ci, c['epi']['store'])
    with Workspace(L, c['ws']):
        core.check(L.ldetr_p3_conv2d_bwd_data(core.ptr(dyp), N, OH, OW, Co, core.ptr(wb), Ci, KH, KW, s, pad, H, W, ctypes.byref(ep), *out.ptrs(), core.stream()), 'bwd_data')
        rec = last_launch(L)
        v = out.value(c['name']).reshape(N, H, W, Ci)
    return v, rec


def launch_wgrad(L, dev, c, t):
    core = _core()
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    xp, dyp = p3_of(L, dev, t['x']), p3_of(L, dev, t['dy'])
    sc = t['row_scale'].to(dev) if c['row_scale'] else None
    dw = Guarded(dev, Co * KH * KW * Ci * 4, init=(t['dw0'] if c['accumulate'] else torch.zeros(Co, KH, KW, Ci)).to(dev))
    core.check(L.ldetr_p3_conv2d_bwd_weight(core.ptr(xp), N, H, W, Ci, core.ptr(dyp), Co, KH, KW, s, pad, core.ptr(sc), dw.ptr(), core.stream()), 'bwd_weight')
    rec = last_launch(L)
    torch.cuda.synchronize()
    dw.check(c['name'] + ' dW')
    return dw.f32().reshape(Co, KH, KW, Ci).clone(), rec


def launch_pair(L, dev, c, t, keep):
    core = _core()
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    OH, OW = P.out_hw(H, W, KH, KW, s, pad)
    dyp, xp, wb = p3_of(L, dev, t['dy']), p3_of(L, dev, t['x']), _weight_bwd(L, dev, c, t)
    sc = t['row_scale'].to(dev) if c['row_scale'] else None
    ep = make_epilogue(L, dev, t, c['epi'], keep)
    out = Out(L, dev, N * H * W, Ci, c['epi']['store'])
    dw = Guarded(dev, Co * KH * KW * Ci * 4, init=(t['dw0'] if c['accumulate'] else torch.zeros(Co, KH, KW, Ci)).to(dev))
    nl = ctypes.c_int(-1)
    with Workspace(L, c['ws']):
        core.check(L.ldetr_p3_conv2d_bwd_pair(core.ptr(dyp), N, OH, OW, Co, core.ptr(wb), core.ptr(xp), Ci, KH, KW, s, pad, H, W, ctypes.byref(ep), *out.ptrs(),
                                              core.ptr(sc), dw.ptr(), ctypes.byref(nl), core.stream()), 'bwd_pair')
        rec = last_launch(L)
        v = out.value(c['name']).reshape(N, H, W, Ci)
    dw.check(c['name'] + ' dW')
    return v, dw.f32().reshape(Co, KH, KW, Ci).clone(), rec, nl.value


# ------------------------------------------------------------------------------------------------------------------------ bars
def expect_model(c, rec):
    if SWEEP_FORCED:
        return
    want, _ = P.model(c, _core().WORKSPACE_BYTES)
    assert rec == want, '%s: the launch policy chose %s, the model says %s' % (c['name'], rec, want)


def hold(c, cls, fam, got, ref, what=''):
    """The class's bar on one output.  ref = (value, pre-activation, sum of |terms|) in float64."""
    v, pre, S = ref
    got = got.detach().cpu()
    if cls != 'rounding':
        bad = P.bit_equal(got, v)
        assert bad == 0, '%s %s %s%s: %d of %d elements differ from float64 (first at %s)' % (
            c['name'], cls, fam, what, bad, v.numel(), ((got != v.float()) & ~(torch.isnan(got) & torch.isnan(v.float()))).nonzero()[0].tolist())
        return
    K = P.reduction_length(c)[fam]
    e, ee = P.rel_err(got, v, S), P.elem_rel_err(got, v, S)
    for key, fig in ((('%s/%d' % (fam, P.k_bucket(K))), e), (('%s_elem/%d' % (fam, P.k_bucket(K))), ee)):
        if fig >= WORST.get(key, (0.0, ''))[0]:
            WORST[key] = (fig, c['name'])
    print('%s %s%s: rel %.2e (bound %.2e)  elem %.2e (bound %.2e)' % (c['name'], fam, what, e, P.bound(fam, K), ee, P.bound(fam, K, True)))
    assert e <= P.bound(fam, K), '%s %s%s: %.2e from float64, bound %.2e' % (c['name'], fam, what, e, P.bound(fam, K))
    assert ee <= P.bound(fam, K, True), '%s %s%s: an element %.2e of its sum of |terms| from float64, bound %.2e' % (c['name'], fam, what, ee, P.bound(fam, K, True))


def _ids(cases):
    return [(c['name'], cls) for c in cases for cls in c['classes']]


def _splitk(rec):
    return rec['splitk'] > 1 or rec['tn_splitk'] > 1


# ------------------------------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize('name,cls', _ids(P.FWD_CASES + P.EPI_CASES), ids=lambda v: v)
def test_forward(dev, L, name, cls):
    rewind(L)
    c, keep = P.BY_NAME[name], []
    t, ref = P.inputs(name, cls), P.reference(name, cls)
    (y,), rec = launch_fwd(L, dev, c, [t], keep)
    expect_model(c, rec)
    hold(c, cls, 'y', y, ref['y'])
    if _splitk(rec):
        rewind(L)
        (y2,), _ = launch_fwd(L, dev, c, [t], keep)
        assert same_bits(y2, y), name + ': the same split-K launch again gives other bits'


@pytest.mark.parametrize('name,cls', _ids(P.DGRAD_CASES), ids=lambda v: v)
def test_data_gradient(dev, L, name, cls):
    rewind(L)
    c, keep = P.BY_NAME[name], []
    t, ref = P.inputs(name, cls), P.reference(name, cls)
    dx, rec = launch_dgrad(L, dev, c, t, keep)
    expect_model(c, rec)
    hold(c, cls, 'dx', dx, ref['dx'])
    if _splitk(rec):
        rewind(L)
        dx2, _ = launch_dgrad(L, dev, c, t, keep)
        assert same_bits(dx2, dx), name + ': the same split-K launch again gives other bits'


@pytest.mark.parametrize('name,cls', _ids(P.WGRAD_CASES), ids=lambda v: v)
def test_weight_gradient(dev, L, name, cls):
    c = P.BY_NAME[name]
    t, ref = P.inputs(name, cls), P.reference(name, cls)
    dw, rec = launch_wgrad(L, dev, c, t)
    expect_model(c, rec)
    hold(c, cls, 'dw', dw, ref['dw'])
    if cls != 'rounding':       # (the order of the pixel slices' atomics is free: only the exact classes repeat bit for bit)
        dw2, _ = launch_wgrad(L, dev, c, t)
        assert same_bits(dw2, dw)


@pytest.mark.parametrize('name,cls', _ids(P.PAIR_CASES), ids=lambda v: v)
def test_paired_backward(dev, L, name, cls):
    """dx bit-equal to the separate launch, dW bit-equal in the exact classes and within the bound in rounding, one launch."""
    rewind(L)
    c, keep = P.BY_NAME[name], []
    t, ref = P.inputs(name, cls), P.reference(name, cls)
    dx, dw, rec, nl = launch_pair(L, dev, c, t, keep)
    expect_model(c, rec)
    if not SWEEP_FORCED:
        assert nl == 1
    hold(c, cls, 'dx', dx, ref['dx'])
    hold(c, cls, 'dw', dw, ref['dw'])
    dx1, _ = launch_dgrad(L, dev, c, t, keep)
    assert same_bits(dx1, dx), name + ': the paired data gradient differs from the separate launch'
    dw1, _ = launch_wgrad(L, dev, c, t)
    if cls != 'rounding':
        assert same_bits(dw1, dw), name + ': the paired weight gradient differs from the separate launch'
    else:
        hold(c, cls, 'dw', dw1, ref['dw'], ' (separate)')
    if _splitk(rec):
        rewind(L)
        dx2, dw2, _, _ = launch_pair(L, dev, c, t, keep)
        assert same_bits(dx2, dx) and (cls == 'rounding' or same_bits(dw2, dw))


@pytest.mark.parametrize('name,cls', _ids(P.DUAL_CASES), ids=lambda v: v)
def test_grouped_forward(dev, L, name, cls):
    """Each set of the grouped launch against its own reference AND bit-equal to its own single launch, with different epilogues and outputs per set."""
    rewind(L)
    c, keep = P.BY_NAME[name], []
    ts = [P.inputs(name, cls, 0), P.inputs(name, cls, 1)]
    refs = [P.reference(name, cls, 0), P.reference(name, cls, 1)]
    ys, rec = launch_fwd(L, dev, c, ts, keep)
    expect_model(c, rec)
    for i in (0, 1):
        hold(c, cls, 'y', ys[i], refs[i]['y'], ' (set %d)' % (i + 1))
        single = dict(c, entry='fwd', epi=c['epi2'] if i else c['epi'], epi2=None)
        (y1,), _ = launch_fwd(L, dev, single, [ts[i]], keep)
        assert same_bits(y1, ys[i]), '%s: set %d of the grouped launch differs from its single launch' % (name, i + 1)
    if _splitk(rec):
        rewind(L)
        ys2, _ = launch_fwd(L, dev, c, ts, keep)
        assert same_bits(ys2[0], ys[0]) and same_bits(ys2[1], ys[1])


# ------------------------------------------------------------------------------------------------------------------------ the cold path
def _classes(t):
    t = t.detach().cpu()
    return torch.isnan(t), torch.isposinf(t), torch.isneginf(t)


def _same_classes(what, got, ref32):
    for nm, a, b in zip(('NaN', '+Inf', '-Inf'), _classes(got), _classes(ref32)):
        assert torch.equal(a, b), '%s: %s positions differ from the fp32 convolution (%d vs %d)' % (what, nm, int(a.sum()), int(b.sum()))
    assert (~torch.isfinite(ref32)).any() and torch.isfinite(ref32).any()


def _finite_bar(c, fam, got, ref64, S, fin):
    got, K = got.detach().cpu().double(), P.reduction_length(c)[fam]
    v = torch.where(fin, ref64, torch.zeros_like(ref64))
    g = torch.where(fin, got, torch.zeros_like(got))
    Sf = torch.where(fin, S, torch.ones_like(S))
    e, ee = P.rel_err(g, v, Sf), P.elem_rel_err(g, v, Sf)
    assert e <= P.bound(fam, K) and ee <= P.bound(fam, K, True), '%s %s: finite outputs %.2e / %.2e from float64' % (c['name'], fam, e, ee)


def _poison_fwd(c, t):
    """+-Inf and NaN at interior pixels and on centre taps only: neither ever meets the zero padding, where 0 x Inf depends on the algorithm."""
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    x, w = t['x'].clone(), t['w'].clone()
    x[0, 3, 4, 5] = float('inf'); x[1 % N, H - 4, 3, 9] = -float('inf'); x[N - 1, 4, W - 4, 0] = float('nan')
    w[3, KH // 2, KW // 2, 7] = float('inf'); w[5, KH // 2, KW // 2, 1] = float('nan'); w[Co - 1, KH // 2, KW // 2, 2] = -float('inf')
    return dict(t, x=x, w=w)


def _poison_dy(c, t):
    N = c['geom'][0]
    dy = t['dy'].clone()
    dy[0, 1, 1, 3] = float('inf'); dy[1 % N, 2, 2, 5] = float('nan'); dy[N - 1, 3, 3, 8] = -float('inf')
    return dict(t, dy=dy)


def _f32_grads(c, t):
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    x = t['x'] if 'x' in t else torch.zeros(N, H, W, Ci)          # (the data gradient does not read x, nor the weight gradient w)
    w = t['w'] if 'w' in t else torch.zeros(Co, KH, KW, Ci)
    xd = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wd = w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv2d(xd, wd, stride=s, padding=pad), (xd, wd), t['dy'].permute(0, 3, 1, 2))
    return gx.permute(0, 2, 3, 1), gw.permute(0, 2, 3, 1)


@pytest.mark.parametrize('name', [c['name'] for c in P.COLD_CASES])
def test_non_finite_operands_on_every_cold_path(dev, L, name):
    """NaN / +Inf / -Inf exactly where torch's fp32 convolution has them, finite outputs at the rounding bar, at every tile and launch kind
    that has a cold path of its own."""
    c, keep = P.BY_NAME[name], []
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    if c['entry'] in ('fwd', 'dual'):
        ts = [_poison_fwd(c, P.inputs(name, 'rounding', i)) for i in ((0, 1) if c['entry'] == 'dual' else (0,))]
        ys, rec = launch_fwd(L, dev, c, ts, keep)
        expect_model(c, rec)
        for t, y in zip(ts, ys):
            ref32 = F.conv2d(t['x'].permute(0, 3, 1, 2), t['w'].permute(0, 3, 1, 2), stride=s, padding=pad).permute(0, 2, 3, 1)
            _same_classes(name, y, ref32)
            acc, S = P.conv_fwd_ref(t['x'], t['w'], s, pad)
            _finite_bar(c, 'y', y, acc, S, torch.isfinite(ref32) & torch.isfinite(acc))
        return
    t = _poison_dy(c, P.inputs(name, 'rounding'))
    gx32, gw32 = _f32_grads(c, t)
    if c['entry'] == 'dgrad':
        dx, rec = launch_dgrad(L, dev, c, t, keep)
        got = dict(dx=dx)
    elif c['entry'] == 'wgrad':
        dw, rec = launch_wgrad(L, dev, c, t)
        got = dict(dw=dw)
    else:
        dx, dw, rec, nl = launch_pair(L, dev, c, t, keep)
        got = dict(dx=dx, dw=dw)
    expect_model(c, rec)
    for fam, g in got.items():
        ref32 = gx32 if fam == 'dx' else gw32
        _same_classes(name + ' ' + fam, g, ref32)
        acc, S = P.conv_dgrad_ref(t['dy'], t['w'], s, pad, H, W) if fam == 'dx' else P.conv_wgrad_ref(t['x'], t['dy'], KH, KW, s, pad)
        _finite_bar(c, fam, g, acc, S, torch.isfinite(ref32) & torch.isfinite(acc))


# ------------------------------------------------------------------------------------------------------------------------ entry guards
@pytest.mark.parametrize('name', [r['name'] for r in P.REJECT_CASES])
def test_entry_guards_reject_without_a_launch(dev, L, name):
    """Every LDETR_CHECK clause of the five conv entries returns LDETR_ERR_ARG and leaves ldetr_p3_last_launch as it was: nothing was launched.
    (The size limits are passed as dimensions: the checks are on the host and come before the launch, so no operand is ever read.)"""
    core = _core()
    r = next(q for q in P.REJECT_CASES if q['name'] == name)
    assert not P.entry_accepts(r['entry'], r['geom'], r['null'], r['oh_delta'])
    # a launch of a known kind first, so that "unchanged" means something
    c0 = P.BY_NAME['f_1x1s1']
    launch_fwd(L, dev, c0, [P.inputs('f_1x1s1', 'grid')], [])
    before = last_launch(L)
    assert before['kind'] == 1
    N, H, W, Ci, Co, KH, KW, s, pad = r['geom']
    OH, OW = P.out_hw(H, W, KH, KW, s, pad)
    OH += r['oh_delta']
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)         # stands in for every operand: never read
    p = lambda k: None if k in r['null'] else core.ptr(buf)
    from layoutdetr_amd import _lib
    ep = _lib.P3Epilogue(); ep.alpha = 1.0
    nl = ctypes.c_int(-1)
    if r['entry'] == 'fwd':
        rc = L.ldetr_p3_conv2d_fwd(p('x'), N, H, W, Ci, p('w'), Co, KH, KW, s, pad, ctypes.byref(ep), p('out'), p('out'), core.stream())
    elif r['entry'] == 'dual':
        rc = L.ldetr_p3_conv2d_fwd_dual(p('x'), p('x2'), N, H, W, Ci, p('w'), p('w2'), Co, KH, KW, s, pad, ctypes.byref(ep), ctypes.byref(ep), p('out'), p('out'),
                                        p('out2'), p('out2'), core.stream())
    elif r['entry'] == 'dgrad':
        rc = L.ldetr_p3_conv2d_bwd_data(p('dy'), N, OH, OW, Co, p('w'), Ci, KH, KW, s, pad, H, W, ctypes.byref(ep), p('out'), p('out'), core.stream())
    elif r['entry'] == 'wgrad':
        rc = L.ldetr_p3_conv2d_bwd_weight(p('x'), N, H, W, Ci, p('dy'), Co, KH, KW, s, pad, None, p('dw'), core.stream())
    else:
        rc = L.ldetr_p3_conv2d_bwd_pair(p('dy'), N, OH, OW, Co, p('w'), p('x'), Ci, KH, KW, s, pad, H, W, ctypes.byref(ep), p('out'), p('out'), None, p('dw'),
                                        ctypes.byref(nl), core.stream())
    assert rc == 1, '%s: return code %d (%s)' % (name, rc, L.ldetr_last_error().decode())
    assert last_launch(L) == before, name + ': a launch happened'
    assert nl.value in (-1, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------ the data gradient's weight image
@pytest.mark.parametrize('shape', [(64, 1, 1, 64), (64, 3, 3, 64), (40, 3, 3, 24), (72, 4, 8, 32), (256, 1, 1, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_weight_bwd_with_scale_is_float32_of_w_times_scale_transposed(dev, L, shape):
    """merge(ldetr_p3_weight_bwd(w, scale)) == float32(w * scale) in [I][T][O] order, bit for bit; the same through ldetr_p3_weight_prep."""
    core = _core()
    O, KH, KW, I = shape
    g = torch.Generator().manual_seed(O * 131 + I)
    w = P.full_mantissa(g, shape, -20, 20)
    sc = P.full_mantissa(g, (O,), -3, 3)
    want = (w.double() * sc.double()[:, None, None, None]).float().reshape(O, KH * KW, I).permute(2, 1, 0).contiguous()        # one rounding, as the fp32 product
    wd, sd = w.to(dev), sc.to(dev)
    img = Guarded(dev, I * KH * KW * O * 6)
    core.check(L.ldetr_p3_weight_bwd(core.ptr(wd), core.ptr(sd), img.ptr(), O, KH, KW, I, core.stream()), 'weight_bwd')
    torch.cuda.synchronize(); img.check('weight_bwd')
    assert torch.equal(p3_merge(L, img.inner, I * KH * KW, O).cpu(), want.reshape(-1, O))
    fwd, bwd = Guarded(dev, w.numel() * 6), Guarded(dev, w.numel() * 6)
    blocks = (w.numel() // 8 + 255) // 256
    table = torch.tensor([[wd.data_ptr(), sd.data_ptr(), fwd.inner.data_ptr(), bwd.inner.data_ptr(), O, KH * KW, I, 0]], dtype=torch.int64, device=dev)
    core.check(L.ldetr_p3_weight_prep(core.ptr(table), 1, blocks, core.stream()), 'prep')
    torch.cuda.synchronize(); fwd.check('weight_prep fwd'); bwd.check('weight_prep bwd')
    assert torch.equal(p3_merge(L, bwd.inner, I * KH * KW, O).cpu(), want.reshape(-1, O))
    assert torch.equal(p3_merge(L, fwd.inner, O * KH * KW, I).cpu(), w.reshape(-1, I))


def test_zz_report_worst_figures():
    """Prints the worst rounding-class figure per output family and reduction-length bucket next to its yardstick and bound (run with -s)."""
    for key in sorted(WORST):
        fam, kb = key.split('/')
        elem = fam.endswith('_elem')
        print('%-14s worst %.2e (%s)  yardstick %.2e  bound %.2e' % (key, WORST[key][0], WORST[key][1], P.FP32_BASELINE[key],
                                                                      P.bound(fam.replace('_elem', ''), int(kb), elem)))
