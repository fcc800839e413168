"""Every path of the token-stack kernels (csrc/mha_small.hip: mha_small_fwd/bwd, mha_cross_fwd/bwd, wgrad_multi; csrc/ffn_fused.hip: ffn_fwd/bwd)
against float64, through their seven C entry points, buffer by buffer.  Tables, references, the path predicates and the measure are in
tests/token_stack_common.py; tests/test_token_stack_ref_cpu.py proves that the tables reach every path, that the exact inputs are exact and that
the references are right and sensitive.  The argument blocks are filled by hip/blocks.py's builders and sent by blocks.launch (the one place that
does so); ldetr_wgrad_multi_f32 gets _lib.WgradDesc descriptors the way hip/stacks.py::_bwd_weights makes them.

Three tiers, each on every buffer a kernel writes (qkv / q, o, lse, ypart, dqkv / dq, dk, dv, h, dh, every part plane, dW, db):
  exact     integer and dyadic inputs: projections, the whole feed-forward, wgrad_multi and the uniform-attention cases EQUAL float64;
  rounding  Gaussian inputs, per (sample, head) / (row tile, hidden slice) block, within 4 x the float32 yardstick and never above the project's
            older bounds (T.bound); every case prints its figures before it asserts;
  footprint outputs are NaN-filled (wgrad's += targets: known values) with guard rows behind them and NaN in every pitch gap: what the header says
            is written is finite, everything else keeps its bits; an optional output passed as NULL leaves the others bit-equal.
Every backward is handed the float64 reference's saved tensors rounded to float32, never the forward kernel's outputs: no share of entries may be
off anywhere.  Two problems in one launch must be bit-equal to the problems launched alone.

Largest measured errors (MI355X; bound = 4 x the float32 yardstick of token_stack_common.FP32_BASELINE): self-attention qkv 3.4e-7 (3.5e-6), o 8.7e-7
(5.5e-6), lse 1.3e-6 (4.5e-6), ypart 9.2e-7 (6.2e-6), dqkv 2.5e-6 (7.2e-6), dxpart 1.2e-6 (6.8e-6); cross-attention q 3.3e-7 (3.1e-6), o 1.2e-6 (5.8e-6),
lse 1.0e-6 (5.1e-6), ypart 1.1e-6 (5.3e-6), dq 2.4e-6 (6.2e-6), dk 2.2e-6 (7.8e-6), dv 1.9e-6 (9.8e-6), dxpart 2.5e-6 (5.7e-6); feed-forward h 4.3e-7
(2.7e-6), ypart 3.5e-7 (2.1e-6), dh 3.8e-7 (3.0e-6), dxpart 4.4e-7 (2.1e-6); wgrad_multi dW 1.5e-7 (1.4e-6), db 1.1e-7 (1.2e-6).  Every exact case equal
(the uniform cases' dv included: expf(-float32(log n)) is 1 / n for n = 1 .. 64), every footprint clean, every grouped launch bit-equal.  44 tests
in 3 s."""
import pytest
import torch

import dropout_common as DC
import token_stack_common as T

pytestmark = pytest.mark.gpu

T.limit_threads()
NAN = float('nan')
GUARD_ROWS = 5
K = T.SEED_NUMBER


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(dev):
    """A device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


def fresh_masks(dev, case):
    """Redraws the device half of the dropout seed (non-zero, pinned to the case) -> the masks the launches of this test will draw."""
    from layoutdetr_amd.hip import core
    torch.manual_seed(0x70C5 + case)
    core.reseed(dev)
    word = core.iter_seed().item()
    assert word != 0
    return DC.Masks(word)


class Figures(object):
    """Collects (name, error, bound) and exact conditions, prints each, asserts them together at the end of a test."""

    def __init__(self):
        self.rows, self.flags = [], []

    def values(self, case, figs):
        self.rows += [(case, key, e, T.bound(key)) for key, e in figs]

    def exact(self, case, name, ok):
        self.flags.append((case, name, bool(ok)))

    def footprint(self, case, outs):
        for name, o in outs.items():
            self.exact(case, f'{name}: every written element finite', o.inside_finite())
            self.exact(case, f'{name}: nothing outside it written (pitch gaps, guard rows)', o.outside_untouched())

    def check(self):
        for case, name, e, tol in self.rows:
            print(f'[token stack] {case}: {name} err {e:.3e} (bound {tol:.2e})')
        for case, name, ok in self.flags:
            print(f'[token stack] {case}: {name}: {"yes" if ok else "NO"}')
        bad = [f'{case} {name}: {e:.3e} > {tol:.2e}' for case, name, e, tol in self.rows if not e <= tol] + \
              [f'{case}: NOT {name}' for case, name, ok in self.flags if not ok]
        assert not bad, '; '.join(bad[:12]) + (f' (+{len(bad) - 12} more)' if len(bad) > 12 else '')


class Out(object):
    """An output buffer of `rows` rows at pitch `ld` with GUARD_ROWS rows behind it (and `lead` floats in front), filled with a sentinel (or `init`,
    [rows, ld]).  windows: (first column, columns) of each view a kernel is given; everything outside the windows must keep its bits."""

    def __init__(self, dev, rows, ld, windows=None, fill=NAN, lead=0, init=None):
        self.full = torch.full((lead + (rows + GUARD_ROWS) * ld,), fill, device=dev)
        body = self.full[lead:].view(rows + GUARD_ROWS, ld)
        if init is not None:
            body[:rows].copy_(init)
        self.inside = torch.zeros_like(self.full, dtype=torch.bool)
        inside = self.inside[lead:].view(rows + GUARD_ROWS, ld)
        self.rows, self.views = rows, []
        for c0, n in (windows or ((0, ld),)):
            inside[:rows, c0:c0 + n] = True
            self.views.append(body[:max(rows, 1), c0:c0 + n])             # (never an empty tensor: its data_ptr() would be NULL)
        self.view = self.views[0]
        self.before = self.full.clone()

    def outside_untouched(self):
        a, b = self.full.view(torch.int32), self.before.view(torch.int32)
        return bool((a[~self.inside] == b[~self.inside]).all())

    def inside_finite(self):
        return bool(self.full[self.inside].isfinite().all())

    def cpu(self, i=0):
        return self.views[i][:self.rows].detach().cpu().clone()


def dev_in(t, dev, pitched=False):
    """An input [rows, cols] on the device inside a NaN-filled buffer with guard rows; pitched: 32 floats of NaN on either side of every row."""
    rows, cols = t.shape
    ld, c0 = (cols + 64, 32) if pitched else (cols, 0)
    buf = torch.full((rows + GUARD_ROWS, ld), NAN, device=dev)
    buf[:rows, c0:c0 + cols].copy_(t)
    return buf[:max(rows, 1), c0:c0 + cols]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def read(outs, shapes):
    return {name: o.cpu().reshape(shapes[name]) if name in shapes else o.cpu() for name, o in outs.items()}


def launch(what, items):
    """items: [(argument block, outputs, shapes)] of 1-2 problems -> their outputs on the CPU."""
    from layoutdetr_amd.hip import blocks
    blocks.launch(what, [a for a, _, _ in items])
    torch.cuda.synchronize()
    return [read(o, s) for _, o, s in items]


def to32(t):
    return t.float()


# ------------------------------------------------------------------------------------------------------------------------ mha_small
class SelfProblem(object):
    def __init__(self, dev, c, kind, masks=None):
        self.dev, self.c, self.kind, self.k = dev, c, kind, K.get(('self', c['name']), 0)
        self.saved = None
        t = self.t = T.self_inputs(c, kind)
        self.x, self.dr = dev_in(t['x'], dev, c['pitched']), dev_in(t['dr'], dev)
        self.w_in, self.b_in, self.w_out = t['w_in'].to(dev), t['b_in'].to(dev), t['w_out'].to(dev)
        self.kpm = t['kpm'].to(torch.uint8).to(dev) if t['kpm'] is not None and c['B'] else None
        if c['p'] > 0:                                                       # the masks of this run's device word
            drop = T.self_drop(c, masks, self.k)
            self.fwd_ref = T.self_fwd_ref(t, c, drop)
            self.bwd_ref, self.mag = T.self_bwd_ref(t, self.fwd_ref, c, drop)
        elif c['B']:
            self.fwd_ref, self.bwd_ref, self.mag = T.self_reference(c['name'], kind, self.k)

    def fwd(self):
        from layoutdetr_amd.hip import blocks
        c, dev = self.c, self.dev
        B, L, M = c['B'], c['L'], c['B'] * c['L']
        outs = dict(qkv=Out(dev, M, 3 * T.D), o=Out(dev, M, T.D), lse=Out(dev, B * T.H, L), ypart=Out(dev, T.H * M, T.D))
        a = blocks.mha_small_fwd(self.x, self.w_in, self.b_in, self.w_out, self.kpm, outs['qkv'].view, outs['o'].view, outs['lse'].view, outs['ypart'].view,
                                 B, L, c['p'], T.host_seed(self.k))
        assert a.ldx == (T.D + 64 if c['pitched'] else T.D)
        return a, outs, dict(lse=(B, T.H, L), ypart=(T.H, M, T.D))

    def bwd(self, dqkv=True):
        from layoutdetr_amd.hip import blocks
        c, dev = self.c, self.dev
        B, L, M = c['B'], c['L'], c['B'] * c['L']
        if self.saved is None and B:                                         # (made once: every launch of this problem reads the same buffers)
            f = self.fwd_ref
            self.saved = [dev_in(to32(f['qkv']), dev), dev_in(to32(f['o']), dev), dev_in(to32(f['lse']).reshape(B * T.H, L), dev)]
        elif self.saved is None:
            self.saved = [dev_in(torch.zeros(0, n), dev) for n in (3 * T.D, T.D, L)]
        outs = dict(dxpart=Out(dev, T.H * M, T.D))
        if dqkv:
            outs['dqkv'] = Out(dev, M, 3 * T.D)
        a = blocks.mha_small_bwd(self.dr, self.w_in, self.w_out, self.kpm, self.saved[0], self.saved[1], self.saved[2], outs['dqkv'].view if dqkv else None,
                                 outs['dxpart'].view, B, L, c['p'], T.host_seed(self.k))
        return a, outs, dict(dxpart=(T.H, M, T.D))


def check_self(fig, tag, c, kind, got_f, got_b, p):
    fig.values(tag, T.self_figures(c, got_f, got_b, p.fwd_ref, p.bwd_ref, p.mag) if kind in T.ROUNDING_KINDS else [])
    if kind in ('dyadic', 'uniform'):
        fig.exact(tag, 'qkv equals float64', torch.equal(got_f['qkv'].double(), p.fwd_ref['qkv']))
    if kind == 'uniform':
        for name in ('o', 'ypart'):
            fig.exact(tag, f'{name} equals float64', torch.equal(got_f[name].double(), p.fwd_ref[name]))
        fig.exact(tag, 'dk and dv (dqkv columns 256..767) equal float64', torch.equal(got_b['dqkv'][:, T.D:].double(), p.bwd_ref['dqkv'][:, T.D:]))


@pytest.mark.parametrize('name', [c['name'] for c in T.SELF_CASES if c['kinds']])
def test_self_attention_every_buffer(dev, name):
    c = T.SELF_BY_NAME[name]
    masks = fresh_masks(dev, K['self', name]) if c['p'] > 0 else None
    fig = Figures()
    for kind in c['kinds']:
        tag = f'self {name} {kind} (paths {sorted(T.self_paths(c))})'
        p = SelfProblem(dev, c, kind, masks)
        fa, fo, fs = p.fwd()
        (got_f,) = launch('mha_small_fwd', [(fa, fo, fs)])
        ba, bo, bs = p.bwd()
        (got_b,) = launch('mha_small_bwd', [(ba, bo, bs)])
        na, no, ns = p.bwd(dqkv=False)
        (got_n,) = launch('mha_small_bwd', [(na, no, ns)])
        fig.footprint(tag, dict(fo, **bo))
        fig.footprint(tag + ' dqkv NULL', no)
        fig.exact(tag, 'dxpart bit-equal with dqkv NULL', same_bits(got_n['dxpart'], got_b['dxpart']))
        check_self(fig, tag, c, kind, got_f, got_b, p)
    fig.check()


@pytest.mark.parametrize('pair', T.SELF_GROUPS, ids=['+'.join(p) for p in T.SELF_GROUPS])
def test_self_attention_two_problems_in_one_launch_equal_the_problems_alone(dev, pair):
    """n = 2: the second problem's blocks follow the first's (nb0 = 8 B of the first, which is 0 for an empty first problem)."""
    cs = [T.SELF_BY_NAME[n] for n in pair]
    masks = fresh_masks(dev, 100 + T.SELF_GROUPS.index(pair))
    ps = [SelfProblem(dev, c, 'gauss', masks) for c in cs]
    fig = Figures()
    tag = f'self group {pair} (paths {sorted(T.self_paths(*cs))})'
    for what, make in (('mha_small_fwd', lambda p: p.fwd()), ('mha_small_bwd', lambda p: p.bwd())):
        alone = [launch(what, [make(p)])[0] if p.c['B'] else None for p in ps]
        items = [make(p) for p in ps]
        both = launch(what, items)
        for i, (p, a, g) in enumerate(zip(ps, alone, both)):
            fig.footprint(f'{tag} {what} problem {i}', items[i][1])
            if a is not None:
                for name in a:
                    fig.exact(tag, f'{what} problem {i} {name} bit-equal to the problem alone', same_bits(a[name], g[name]))
    for p in ps:                                  # ... and right: the grouped launch's values against float64 come through the single-problem test
        assert p.c['B'] == 0 or p.c['kinds']
    fig.check()


def test_self_attention_empty_problem_alone_launches_nothing(dev):
    p = SelfProblem(dev, T.SELF_BY_NAME['L10-B0'], 'gauss')
    fig = Figures()
    for what, item in (('mha_small_fwd', p.fwd()), ('mha_small_bwd', p.bwd())):
        launch(what, [item])                      # returns LDETR_OK (blocks.launch raises otherwise)
        fig.footprint(f'self B = 0 {what} (paths {sorted(T.self_paths(p.c))})', item[1])
    fig.check()


def _without_sample(t, name, B, L, gone=1):
    """A buffer of B samples without sample `gone`: lse [B, 8, L], part planes [8, B*L, 256], rows [B*L, C]."""
    keep = [b for b in range(B) if b != gone]
    if name in ('lse', 'mag_lse'):
        return t[keep]
    if name in ('ypart', 'dxpart'):
        return t.reshape(T.H, B, L, T.D)[:, keep].reshape(T.H, -1, T.D)
    return t.reshape(B, L, -1)[keep].reshape(len(keep) * L, -1)


def _nan_report(t):
    return f'{int(t.isnan().sum())} NaN, {int((t == 0).sum())} zeros of {t.numel()}'


def test_self_attention_fully_masked_sample_is_isolated(dev):
    """Sample 1 of 3 has every key masked.  Forward: its o and ypart rows are NaN exactly where float64's are (softmax of a row of -inf), every other
    sample is within the bounds.  Backward, handed the reference's saved tensors (NaN o and -inf lse for that sample): every other sample within the
    bounds.  Nothing is asserted about the masked sample's own backward rows: the kernel's p is 0 for a masked key, so its dv rows are 0, and
    delta = o . dO is NaN, so its dq, dk and dxpart rows are NaN; the reference's p = exp(-inf - -inf) is NaN, so all of its rows are NaN (printed)."""
    c = T.SELF_MASKED
    B, L = c['B'], c['L']
    p = SelfProblem(dev, c, 'gauss')
    (got_f,), (got_b,) = launch('mha_small_fwd', [p.fwd()]), launch('mha_small_bwd', [p.bwd()])
    fig = Figures()
    tag = f'self {c["name"]}'
    for name in ('o', 'ypart'):
        fig.exact(tag, f'{name} NaN exactly where float64 is', torch.equal(got_f[name].isnan(), p.fwd_ref[name].isnan()) and bool(p.fwd_ref[name].isnan().any()))
    c2 = dict(c, B=B - 1)
    cut = lambda d: {n: _without_sample(v, n, B, L) for n, v in d.items()}
    fig.values(tag + ' other samples', T.self_figures(c2, cut(got_f), cut(got_b), cut(p.fwd_ref), cut(p.bwd_ref), cut(p.mag)))
    rows = slice(L, 2 * L)
    print(f'[token stack] {tag}: masked sample backward rows, kernel: dq {_nan_report(got_b["dqkv"][rows, :T.D])}; dk {_nan_report(got_b["dqkv"][rows, T.D:2 * T.D])}; '
          f'dv {_nan_report(got_b["dqkv"][rows, 2 * T.D:])}; dxpart {_nan_report(got_b["dxpart"][:, rows])}; reference: dqkv {_nan_report(p.bwd_ref["dqkv"][rows])}')
    fig.check()


# ------------------------------------------------------------------------------------------------------------------------ mha_cross
class CrossProblem(object):
    def __init__(self, dev, c, kind, masks=None):
        self.dev, self.c, self.kind, self.k = dev, c, kind, K.get(('cross', c['name']), 0)
        self.saved = None
        t = self.t = T.cross_inputs(c, kind)
        Mk = c['B'] * c['Lk']
        self.x, self.dr = dev_in(t['x'], dev), dev_in(t['dr'], dev)
        if c['pitched']:                                                     # k and v as views into one wider buffer, the way grouped_kv makes them
            kv = torch.full((Mk + GUARD_ROWS, 640), NAN, device=dev)
            self.kk, self.v = kv[:Mk, 64:320], kv[:Mk, 384:640]
            self.kk.copy_(t['k']); self.v.copy_(t['v'])
        else:
            self.kk, self.v = dev_in(t['k'], dev), dev_in(t['v'], dev)
        self.w_q, self.b_q, self.w_out = t['w_q'].to(dev), t['b_q'].to(dev), t['w_out'].to(dev)
        self.kpm = t['kpm'].to(torch.uint8).to(dev) if t['kpm'] is not None else None
        if c['p'] > 0:
            drop = T.cross_drop(c, masks, self.k)
            self.fwd_ref = T.cross_fwd_ref(t, c, drop)
            self.bwd_ref, self.mag = T.cross_bwd_ref(t, self.fwd_ref, c, drop)
        else:
            self.fwd_ref, self.bwd_ref, self.mag = T.cross_reference(c['name'], kind, self.k)

    def fwd(self):
        from layoutdetr_amd.hip import blocks
        c, dev = self.c, self.dev
        B, Lq, Lk, Mq = c['B'], c['Lq'], c['Lk'], c['B'] * c['Lq']
        outs = dict(q=Out(dev, Mq, T.D), o=Out(dev, Mq, T.D), lse=Out(dev, B * T.H, Lq), ypart=Out(dev, T.H * Mq, T.D))
        a = blocks.mha_cross_fwd(self.x, self.w_q, self.b_q, self.kk, self.v, self.w_out, self.kpm, outs['q'].view, outs['o'].view, outs['lse'].view,
                                 outs['ypart'].view, B, Lq, Lk, c['p'], T.host_seed(self.k))
        assert a.ldk == a.ldv == (640 if c['pitched'] else T.D)
        return a, outs, dict(lse=(B, T.H, Lq), ypart=(T.H, Mq, T.D))

    def bwd(self):
        from layoutdetr_amd.hip import blocks
        c, dev, f = self.c, self.dev, self.fwd_ref
        B, Lq, Lk, Mq, Mk = c['B'], c['Lq'], c['Lk'], c['B'] * c['Lq'], c['B'] * c['Lk']
        if self.saved is None:
            self.saved = [dev_in(to32(f['q']), dev), dev_in(to32(f['o']), dev), dev_in(to32(f['lse']).reshape(B * T.H, Lq), dev)]
        outs = dict(dq=Out(dev, Mq, T.D), dxpart=Out(dev, T.H * Mq, T.D))
        if c['pitched']:
            outs['dkdv'] = Out(dev, Mk, 640, windows=((64, T.D), (384, T.D)))
            dk, dv = outs['dkdv'].views
        else:
            outs['dk'], outs['dv'] = Out(dev, Mk, T.D), Out(dev, Mk, T.D)
            dk, dv = outs['dk'].view, outs['dv'].view
        a = blocks.mha_cross_bwd(self.dr, self.w_q, self.kk, self.v, self.w_out, self.kpm, self.saved[0], self.saved[1], self.saved[2], outs['dq'].view, dk, dv,
                                 outs['dxpart'].view, B, Lq, Lk, c['p'], T.host_seed(self.k))
        assert a.lddk == a.lddv == (640 if c['pitched'] else T.D) and a.dq
        return a, outs, dict(dxpart=(T.H, Mq, T.D))


def run_cross(p):
    (got_f,) = launch('mha_cross_fwd', [p.fwd()])
    item = p.bwd()
    (got_b,) = launch('mha_cross_bwd', [item])
    if 'dkdv' in got_b:
        got_b['dk'], got_b['dv'] = item[1]['dkdv'].cpu(0), item[1]['dkdv'].cpu(1)
        del got_b['dkdv']
    return got_f, got_b, item[1]


@pytest.mark.parametrize('name', [c['name'] for c in T.CROSS_CASES])
def test_cross_attention_every_buffer(dev, name):
    c = T.CROSS_BY_NAME[name]
    masks = fresh_masks(dev, K['cross', name]) if c['p'] > 0 else None
    fig = Figures()
    for kind in c['kinds']:
        tag = f'cross {name} {kind} (paths {sorted(T.cross_paths(c))})'
        p = CrossProblem(dev, c, kind, masks)
        fitem = p.fwd()
        (got_f,) = launch('mha_cross_fwd', [fitem])
        _, got_b, bouts = run_cross(p)
        fig.footprint(tag, dict(fitem[1], **bouts))
        fig.values(tag, T.cross_figures(c, got_f, got_b, p.fwd_ref, p.bwd_ref, p.mag) if kind in T.ROUNDING_KINDS else [])
        if kind in ('dyadic', 'uniform'):
            fig.exact(tag, 'q equals float64', torch.equal(got_f['q'].double(), p.fwd_ref['q']))
        if kind == 'uniform':
            for name_ in ('o', 'ypart'):
                fig.exact(tag, f'{name_} equals float64', torch.equal(got_f[name_].double(), p.fwd_ref[name_]))
            for name_ in ('dk', 'dv'):
                fig.exact(tag, f'{name_} equals float64', torch.equal(got_b[name_].double(), p.bwd_ref[name_]))
    fig.check()


def test_cross_attention_fully_masked_sample_is_isolated(dev):
    """As test_self_attention_fully_masked_sample_is_isolated, onto 33 memory tokens.  The masked sample's own backward rows (not asserted): the
    kernel's dv rows are 0 (p = 0 for a masked key) and its dq, dk and dxpart rows NaN (delta = o . dO with the NaN o); the reference's are all NaN."""
    c = T.CROSS_MASKED
    B, Lq, Lk = c['B'], c['Lq'], c['Lk']
    p = CrossProblem(dev, c, 'gauss')
    got_f, got_b, _ = run_cross(p)
    fig = Figures()
    tag = f'cross {c["name"]}'
    for name in ('o', 'ypart'):
        fig.exact(tag, f'{name} NaN exactly where float64 is', torch.equal(got_f[name].isnan(), p.fwd_ref[name].isnan()) and bool(p.fwd_ref[name].isnan().any()))
    c2 = dict(c, B=B - 1)
    cut = lambda d: {n: _without_sample(v, n, B, Lk if n in ('dk', 'dv') else Lq) for n, v in d.items()}
    fig.values(tag + ' other samples', T.cross_figures(c2, cut(got_f), cut(got_b), cut(p.fwd_ref), cut(p.bwd_ref), cut(p.mag)))
    print(f'[token stack] {tag}: masked sample backward rows, kernel: dq {_nan_report(got_b["dq"][Lq:2 * Lq])}; dk {_nan_report(got_b["dk"][Lk:2 * Lk])}; '
          f'dv {_nan_report(got_b["dv"][Lk:2 * Lk])}; dxpart {_nan_report(got_b["dxpart"][:, Lq:2 * Lq])}; reference: dq {_nan_report(p.bwd_ref["dq"][Lq:2 * Lq])}, '
          f'dk {_nan_report(p.bwd_ref["dk"][Lk:2 * Lk])}, dv {_nan_report(p.bwd_ref["dv"][Lk:2 * Lk])}')
    fig.check()


# ------------------------------------------------------------------------------------------------------------------------ feed-forward
class FfnProblem(object):
    def __init__(self, dev, c, kind, masks=None):
        self.dev, self.c, self.kind, self.k = dev, c, kind, K['ffn', c['name']]
        self.saved = None
        t = self.t = T.ffn_inputs(c, kind)
        self.x, self.dy = dev_in(t['x'], dev, c['pitched']), dev_in(t['dy'], dev)
        self.w1, self.b1, self.w2 = t['w1'].to(dev), t['b1'].to(dev), t['w2'].to(dev)
        if c['p'] > 0:
            self.fwd_ref = T.ffn_fwd_ref(t, c, T.ffn_drop(c, masks, self.k))
            self.bwd_ref = T.ffn_bwd_ref(t, self.fwd_ref, c)
        else:
            self.fwd_ref, self.bwd_ref = T.ffn_reference(c['name'], kind, self.k)

    def fwd(self):
        from layoutdetr_amd.hip import blocks
        c, dev = self.c, self.dev
        M, F = c['M'], c['F']
        outs = dict(h=Out(dev, M, F), ypart=Out(dev, F // T.FHS * M, T.D))
        a = blocks.ffn_fwd(self.x, self.w1, self.b1, self.w2, outs['h'].view, outs['ypart'].view, c['p'], T.host_seed(self.k))
        assert (a.M, a.F, a.ldx) == (M, F, T.D + 64 if c['pitched'] else T.D)
        return a, outs, dict(ypart=(F // T.FHS, M, T.D))

    def bwd(self, dh=True):
        from layoutdetr_amd.hip import blocks
        c, dev = self.c, self.dev
        M, F = c['M'], c['F']
        if self.saved is None:
            self.saved = dev_in(to32(self.fwd_ref['h']), dev)
        outs = dict(dxpart=Out(dev, F // T.FHS * M, T.D))
        if dh:
            outs['dh'] = Out(dev, M, F)
        a = blocks.ffn_bwd(self.dy, self.x, self.saved, self.w1, self.w2, outs['dxpart'].view, outs['dh'].view if dh else None, c['p'])
        return a, outs, dict(dxpart=(F // T.FHS, M, T.D))


@pytest.mark.parametrize('name', [c['name'] for c in T.FFN_CASES])
def test_feed_forward_every_buffer(dev, name):
    c = T.FFN_BY_NAME[name]
    masks = fresh_masks(dev, K['ffn', name]) if c['p'] > 0 else None
    fig = Figures()
    for kind in c['kinds']:
        tag = f'ffn {name} {kind} (paths {sorted(T.ffn_paths(c))})'
        p = FfnProblem(dev, c, kind, masks)
        fitem, bitem, nitem = p.fwd(), p.bwd(), p.bwd(dh=False)
        (got_f,), (got_b,), (got_n,) = launch('ffn_fwd', [fitem]), launch('ffn_bwd', [bitem]), launch('ffn_bwd', [nitem])
        fig.footprint(tag, dict(fitem[1], **bitem[1]))
        fig.footprint(tag + ' dh NULL', nitem[1])
        fig.exact(tag, 'dxpart bit-equal with dh NULL', same_bits(got_n['dxpart'], got_b['dxpart']))
        if kind == 'gauss':
            fig.values(tag, T.ffn_figures(c, got_f, got_b, p.fwd_ref, p.bwd_ref))
        else:
            for name_, got, ref in (('h', got_f, p.fwd_ref), ('ypart', got_f, p.fwd_ref), ('dh', got_b, p.bwd_ref), ('dxpart', got_b, p.bwd_ref)):
                fig.exact(tag, f'{name_} equals float64', torch.equal(got[name_].double(), ref[name_]))
        # the mask the backward applied is the saved h's, entry for entry: no share of entries may differ
        fig.exact(tag, 'dh is 0 exactly where the saved h is 0', torch.equal(got_b['dh'] == 0, (p.fwd_ref['h'].float() == 0) | (p.bwd_ref['dh'] == 0)))
    fig.check()


@pytest.mark.parametrize('pair', T.FFN_GROUPS, ids=['+'.join(p) for p in T.FFN_GROUPS])
def test_feed_forward_two_problems_in_one_launch_equal_the_problems_alone(dev, pair):
    cs = [T.FFN_BY_NAME[n] for n in pair]
    masks = fresh_masks(dev, 200 + T.FFN_GROUPS.index(pair))
    ps = [FfnProblem(dev, c, 'gauss', masks) for c in cs]
    fig = Figures()
    tag = f'ffn group {pair} (paths {sorted(T.ffn_paths(*cs))})'
    for what, make in (('ffn_fwd', lambda p: p.fwd()), ('ffn_bwd', lambda p: p.bwd())):
        alone = [launch(what, [make(p)])[0] for p in ps]
        items = [make(p) for p in ps]
        both = launch(what, items)
        for i, (a, g) in enumerate(zip(alone, both)):
            fig.footprint(f'{tag} {what} problem {i}', items[i][1])
            for name in a:
                fig.exact(tag, f'{what} problem {i} {name} bit-equal to the problem alone', same_bits(a[name], g[name]))
    fig.check()


# ------------------------------------------------------------------------------------------------------------------------ wgrad_multi
def run_wgrad(dev, group, kind, gi, with_db=True):
    """One ldetr_wgrad_multi_f32 call over the group's descriptors, filled as hip/stacks.py::_bwd_weights fills them -> [(inputs, dW Out, db Out)]."""
    from layoutdetr_amd import _lib
    from layoutdetr_amd.hip import core
    descs, state, keep = [], [], []
    for i, d in enumerate(group):
        t = T.wgrad_inputs(d, kind, 16 * gi + i)
        A, Bm = dev_in(t['A'], dev), dev_in(t['B'], dev)
        Av = A[:, d['a_col0']:d['a_col0'] + d['rows']]
        dW = Out(dev, d['rows'], d['ldw'], windows=((0, d['cols']),), lead=d['dw_off'], init=t['dW0'])
        db = Out(dev, 1, d['rows'], init=t['db0'][None]) if d['db'] and with_db else None
        q = _lib.WgradDesc()
        q.A, q.lda, q.B, q.ldb, q.dW, q.ldw, q.db = Av.data_ptr(), A.stride(0), Bm.data_ptr(), Bm.stride(0), dW.view.data_ptr(), d['ldw'], db.view.data_ptr() if db else None
        q.M, q.rows, q.cols = d['M'], d['rows'], d['cols']
        assert q.A and q.B and q.dW and dW.view.data_ptr() % 16 == 4 * (d['dw_off'] % 4)
        descs.append(q); state.append((t, dW, db)); keep += [A, Bm]
    arr = (_lib.WgradDesc * len(descs))(*descs)
    core.check(core.lib().ldetr_wgrad_multi_f32(arr, len(descs), core.stream()), 'wgrad_multi')
    torch.cuda.synchronize()
    return state


@pytest.mark.parametrize('gname', list(T.WGRAD_GROUPS))
def test_wgrad_multi_every_descriptor(dev, gname):
    group, gi = T.WGRAD_GROUPS[gname], list(T.WGRAD_GROUPS).index(gname)
    fig = Figures()
    for kind in ('dyadic', 'gauss'):
        state, nodb = run_wgrad(dev, group, kind, gi), run_wgrad(dev, group, kind, gi, with_db=False)
        for i, (d, (t, dW, db), (_, dW2, _)) in enumerate(zip(group, state, nodb)):
            tag = f'wgrad {gname}[{i}] M{d["M"]} {d["rows"]}x{d["cols"]} {kind} (group paths {sorted(T.wgrad_paths(group))})'
            ref = T.wgrad_ref(t, d)
            got = dict(dw=dW.cpu(), db=db.cpu()[0] if db else ref['db'])          # (no db: nothing to compare)
            fig.footprint(tag, dict(dW=dW, **({'db': db} if db else {})))
            fig.exact(tag, 'dW bit-equal with every db NULL', same_bits(dW2.cpu(), dW.cpu()))
            if kind == 'gauss':
                fig.values(tag, T.wgrad_figures(d, got, ref))
            else:
                fig.exact(tag, 'dW (its prior content included) equals float64', torch.equal(got['dw'].double(), ref['dw'][:, :d['cols']]))
                fig.exact(tag, 'db (its prior content included) equals float64', torch.equal(got['db'].double(), ref['db']))
            if d['M'] == 0:
                fig.exact(tag, 'an M = 0 descriptor changes nothing', same_bits(dW.full, dW.before) and (db is None or same_bits(db.full, db.before)))
    fig.check()
