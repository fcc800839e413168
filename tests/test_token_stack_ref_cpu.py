"""No GPU: what tests/test_token_stack_gpu.py relies on.  The case tables of tests/token_stack_common.py reach every path name of the four families
(the predicates restate the host side of csrc/mha_small.hip and csrc/ffn_fused.hip) and every size the kernels treat differently; the exact-tier
inputs really make every partial sum a float32; the recorded float32 yardsticks are what this machine measures; each mistake the suite claims to
catch moves a checked buffer by more than 100 x its bound; and the per-kernel references, with the part planes summed and the bias added, are
oracle/detr_ref.py's attention and feed-forward."""
import math

import numpy as np
import pytest
import torch

import dropout_common as DC
import token_stack_common as T
from oracle import detr_ref

T.limit_threads()
MASKS = DC.Masks(T.WORD)
FACTOR = 100.0
K = T.SEED_NUMBER
EXACT_SCALE = 1.0 / math.sqrt(T.DH)           # the oracle's; T.SCALE is its float32 rounding, which the kernels are handed


# ------------------------------------------------------------------------------------------------------------------------ path coverage
def _family_paths(family):
    if family == 'self':
        named = [(c['name'], T.self_paths(c)) for c in T.SELF_CASES]
        named += [(f'{a}+{b}', T.self_paths(T.SELF_BY_NAME[a], T.SELF_BY_NAME[b])) for a, b in T.SELF_GROUPS]
        return named, T.SELF_PATHS
    if family == 'cross':
        return [(c['name'], T.cross_paths(c)) for c in T.CROSS_CASES], T.CROSS_PATHS
    if family == 'ffn':
        named = [(c['name'], T.ffn_paths(c)) for c in T.FFN_CASES]
        named += [(f'{a}+{b}', T.ffn_paths(T.FFN_BY_NAME[a], T.FFN_BY_NAME[b])) for a, b in T.FFN_GROUPS]
        return named, T.FFN_PATHS
    return [(name, T.wgrad_paths(g)) for name, g in T.WGRAD_GROUPS.items()], T.WGRAD_PATHS


@pytest.mark.parametrize('family', ['self', 'cross', 'ffn', 'wgrad'])
def test_every_path_is_reached_and_none_is_unknown(family):
    named, paths = _family_paths(family)
    assert len(set(paths)) == len(paths)
    seen = set()
    for name, names in named:
        assert names, name
        assert not names - set(paths), f'{family} {name}: unknown path {sorted(names - set(paths))}'
        seen |= names
    assert not [p for p in paths if p not in seen], f'{family}: no case takes {[p for p in paths if p not in seen]}'


def test_tables_hold_every_size_the_kernels_treat_differently():
    run = lambda cases: [c for c in cases if c['kinds']]
    assert {c['L'] for c in run(T.SELF_CASES)} >= {1, 9, 10, 15, 16} and {c['B'] for c in T.SELF_CASES} >= {0, 1, 3}
    assert {c['kpm'] for c in T.SELF_CASES} >= {'none', 'ragged', 'key0'}
    assert any(c['pitched'] for c in T.SELF_CASES) and sum(c['p'] > 0 for c in T.SELF_CASES) == 1
    firsts, seconds = [T.SELF_BY_NAME[a] for a, _ in T.SELF_GROUPS], [T.SELF_BY_NAME[b] for _, b in T.SELF_GROUPS]
    assert any(a['B'] == 0 for a in firsts) and any(b['B'] == 0 for b in seconds)
    assert any(a['B'] and b['B'] and a['B'] != b['B'] and a['L'] != b['L'] and a['kpm'] == 'none' and b['kpm'] != 'none' for a, b in zip(firsts, seconds))
    assert {c['Lq'] for c in T.CROSS_CASES} >= {1, 9, 16} and {c['Lk'] for c in T.CROSS_CASES} >= {1, 15, 16, 17, 33, 48, 64}
    assert {c['kpm'] for c in T.CROSS_CASES} >= {'none', 'ragged', 'midtile'} and sum(c['p'] > 0 for c in T.CROSS_CASES) == 1
    assert {c['pitched'] for c in T.CROSS_CASES} == {False, True}
    assert {c['M'] for c in T.FFN_CASES} >= {1, 31, 32, 33, 70} and {c['F'] for c in T.FFN_CASES} >= {64, 128, 320}
    assert {c['pitched'] for c in T.FFN_CASES} == {False, True} and sum(c['p'] > 0 for c in T.FFN_CASES) == 1
    assert any(T.FFN_BY_NAME[a]['M'] != T.FFN_BY_NAME[b]['M'] and T.FFN_BY_NAME[a]['F'] != T.FFN_BY_NAME[b]['F'] for a, b in T.FFN_GROUPS)
    descs = [d for g in T.WGRAD_GROUPS.values() for d in g]
    assert {len(g) for g in T.WGRAD_GROUPS.values()} >= {1, 3, 8} and {d['M'] for d in descs} >= {0, 1, 15, 16, 17, 70}
    assert all(any(d['M'] == 0 for d in g) and any(d['M'] > 0 for d in g) for g in (T.WGRAD_GROUPS['n3'], T.WGRAD_GROUPS['n8']))
    # within the entry points' checks (csrc/mha_small.hip:824, :860, :898; csrc/ffn_fused.hip:216) and the issue's size limits
    assert all(1 <= c['L'] <= 16 for c in T.SELF_CASES) and all(1 <= c['Lq'] <= 16 and 1 <= c['Lk'] <= 64 for c in T.CROSS_CASES)
    assert all(c['F'] % 64 == 0 and c['F'] <= 320 and c['M'] <= 70 for c in T.FFN_CASES) and all(d['M'] <= 70 for d in descs)


def test_masks_are_ragged_and_single_key_and_power_of_two_where_the_tables_say_so():
    for c in T.SELF_CASES + T.CROSS_CASES + [T.SELF_MASKED, T.CROSS_MASKED]:
        Lk = c.get('Lk', c.get('L'))
        kpm = T.make_kpm(c['kpm'], c['B'], Lk, Lk)
        if kpm is None:
            continue
        kept = (~kpm).sum(1)
        if c['kpm'] == 'full':
            assert kept[1] == 0 and kept[0] > 0 and kept[2] > 0
            continue
        assert bool((kept >= 1).all()), c['name']
        if c['kpm'] == 'key0':
            assert kept[1 % c['B']] == 1 and not kpm[1 % c['B'], 0]
        if c['kpm'] == 'midtile':
            assert bool(kpm[1 % c['B'], 16:32].all()) and not bool(kpm[1 % c['B'], :16].all()) and not bool(kpm[1 % c['B'], 32:].all())
        if c['kpm'] == 'pow2':
            assert all(int(n) & (int(n) - 1) == 0 for n in kept) and len(set(kept.tolist())) == c['B'], c['name']
        if c['kpm'] == 'ragged' and Lk >= 9 and c['B'] > 1:
            assert len(set(kept.tolist())) > 1 and bool(kpm.any()), c['name']


# ------------------------------------------------------------------------------------------------------------------------ exact-tier preconditions
LIMIT = 2.0 ** 24


def _abs_inputs(t):
    return {k_: (v.abs() if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k_, v in t.items()}


def _exact(ref, sum_abs_terms, quantum, what):
    """Every partial sum is a multiple of `quantum` below 2^24 quanta, and the float64 result is a float32."""
    assert float(sum_abs_terms.max()) / quantum < LIMIT, f'{what}: {float(sum_abs_terms.max()) / quantum:.3g} quanta'
    assert torch.equal(ref / quantum, (ref / quantum).round()), f'{what}: not a multiple of {quantum}'
    assert torch.equal(ref.float().double(), ref), f'{what}: the float64 result is no float32'


def test_rounded_lse_of_a_power_of_two_gives_back_one_over_n():
    """The uniform cases' backward: the kernel forms p = expf(0 - float32(log n)); the rounded log is within 2^-25 of log n, half the spacing of the
    float32s below 1 / n, so 1 / n is the correctly rounded result (what the exact reference uses)."""
    for n in (1, 2, 4, 8, 16, 32, 64):
        lse = float(np.float32(math.log(n)))
        assert abs(lse - math.log(n)) < 2.0 ** -25 and float(np.float32(math.exp(-lse))) == 1.0 / n


@pytest.mark.parametrize('c', [c for c in T.SELF_CASES if 'dyadic' in c['kinds']] + [c for c in T.CROSS_CASES if 'dyadic' in c['kinds']], ids=lambda c: c['name'])
def test_dyadic_projection_inputs_make_every_partial_sum_a_float32(c):
    if 'L' in c:
        t = T.self_inputs(c, 'dyadic')
        ref, big = T.self_reference(c['name'], 'dyadic', K['self', c['name']])[0]['qkv'], t['x'].abs().double() @ t['w_in'].abs().double().t() + t['b_in'].abs().double()
    else:
        t = T.cross_inputs(c, 'dyadic')
        ref, big = T.cross_reference(c['name'], 'dyadic', K['cross', c['name']])[0]['q'], t['x'].abs().double() @ t['w_q'].abs().double().t() + t['b_q'].abs().double()
    _exact(ref, big, 0.25, c['name'])
    assert bool((ref != 0).any())


@pytest.mark.parametrize('c', [c for c in T.SELF_CASES + T.CROSS_CASES if 'uniform' in c['kinds']], ids=lambda c: c['name'])
def test_uniform_attention_inputs_make_o_ypart_dk_dv_exact(c):
    own = 'L' in c
    Lq, Lk = (c['L'], c['L']) if own else (c['Lq'], c['Lk'])
    t = (T.self_inputs if own else T.cross_inputs)(c, 'uniform')
    fwd, bwd, _ = (T.self_reference if own else T.cross_reference)(c['name'], 'uniform', K['self' if own else 'cross', c['name']])
    ta = _abs_inputs(t)
    fa = (T.self_fwd_ref if own else T.cross_fwd_ref)(ta, c)        # the same sums over |terms|: the scores are still 0
    kept = Lk if t['kpm'] is None else int((~t['kpm']).sum(1).max())
    assert kept & (kept - 1) == 0
    scores = T._scores(fwd['qkv'][:, :T.D] if own else fwd['q'], fwd['qkv'][:, T.D:2 * T.D] if own else t['k'].double(), None, c['B'], Lq, Lk, T.SCALE)
    assert bool((scores == 0).all())
    _exact(fwd['qkv'] if own else fwd['q'], fa['qkv'] if own else fa['q'], 0.25, 'projection')
    vq = 0.25 if own else 1.0                                        # quantum of v
    _exact(fwd['o'], fa['o'], vq / kept, 'o')
    _exact(fwd['ypart'], fa['ypart'], vq / kept / 4, 'ypart')
    dO_abs = ta['dr'].double() @ ta['w_out'].double()
    dv_abs = Lq * dO_abs.max()                                       # p <= 1: at most Lq terms, each at most |dO|
    dk, dv = (bwd['dqkv'][:, T.D:2 * T.D], bwd['dqkv'][:, 2 * T.D:]) if own else (bwd['dk'], bwd['dv'])
    _exact(dv, dv_abs, 0.25 / kept, 'dv')
    assert bool((dk == 0).all()) and bool((dv != 0).any()) and bool((fwd['o'] != 0).any())
    # the rounded lse the kernel's backward is handed gives the same p up to rounding: the two references differ by rounding noise alone
    approx = (T.self_bwd_ref if own else T.cross_bwd_ref)(t, fwd, c)[0]
    assert T.block_err(approx['dqkv'][:, 2 * T.D:] if own else approx['dv'], dv, T.blk_rows(c['B'], Lk)) < 2e-8


@pytest.mark.parametrize('c', [c for c in T.FFN_CASES if 'dyadic' in c['kinds']], ids=lambda c: c['name'])
def test_dyadic_feed_forward_inputs_make_every_buffer_exact(c):
    t = T.ffn_inputs(c, 'dyadic')
    fwd, bwd = T.ffn_reference(c['name'], 'dyadic', K['ffn', c['name']])
    ta = _abs_inputs(t)
    fa = T.ffn_fwd_ref(ta, c)
    ba = T.ffn_bwd_ref(ta, fa, c)
    for name, ref, big, q in (('h', fwd['h'], fa['h'], 0.25), ('ypart', fwd['ypart'], fa['ypart'], 1 / 16), ('dh', bwd['dh'], ba['dh'], 0.25),
                              ('dxpart', bwd['dxpart'], ba['dxpart'], 1 / 16)):
        _exact(ref, big, q, f'{c["name"]} {name}')
    assert 0.2 < float((fwd['h'] > 0).double().mean()) < 0.8, 'the relu must cut some units and pass others'


def test_integer_wgrad_inputs_make_every_partial_sum_a_float32():
    for gi, (name, group) in enumerate(T.WGRAD_GROUPS.items()):
        for i, d in enumerate(group):
            t = T.wgrad_inputs(d, 'dyadic', 16 * gi + i)
            ref = T.wgrad_ref(t, d)
            _exact(ref['dw'], T.wgrad_ref(_abs_inputs(t), d)['dw'], 1.0, f'{name}[{i}] dW')
            _exact(ref['db'], T.wgrad_ref(_abs_inputs(t), d)['db'], 1.0, f'{name}[{i}] db')
            assert bool((t['dW0'] != 0).any()) and (d['M'] == 0 or not torch.equal(ref['dw'], t['dW0'].double()))


# ------------------------------------------------------------------------------------------------------------------------ the float32 yardstick
def test_recorded_fp32_baselines_are_what_this_machine_measures():
    got = T.measure_fp32_baselines()
    print('FP32_BASELINE = dict(' + ', '.join(f'{k_}={v:.2e}' for k_, v in got.items()) + ')')
    assert set(got) == set(T.FP32_BASELINE)
    bad = [f'{k_}: recorded {T.FP32_BASELINE[k_]:.2e}, measured {v:.2e}' for k_, v in got.items() if not T.FP32_BASELINE[k_] / 4 <= v <= T.FP32_BASELINE[k_] * 4]
    assert not bad, '; '.join(bad)
    assert all(T.bound(k_) <= T.PROJECT_BOUND[k_] for k_ in got)


def test_gauss_scores_are_spread_out():
    """The rounding tier's softmax is not flat: the scores of every attention case with more than one key have a standard deviation above 1."""
    for c in T.SELF_CASES:
        if 'gauss' in c['kinds'] and c['L'] > 1:
            f = T.self_reference(c['name'], 'gauss', K['self', c['name']])[0]
            s = T._scores(f['qkv'][:, :T.D], f['qkv'][:, T.D:2 * T.D], None, c['B'], c['L'], c['L'], T.SCALE)
            assert float(s.std()) > 1.0, c['name']
    for c in T.CROSS_CASES:
        if 'gauss' in c['kinds'] and c['Lk'] > 1:
            f = T.cross_reference(c['name'], 'gauss', K['cross', c['name']])[0]
            s = T._scores(f['q'], T.cross_inputs(c, 'gauss')['k'].double(), None, c['B'], c['Lq'], c['Lk'], T.SCALE)
            assert float(s.std()) > 1.0, c['name']


def test_block_measure_sees_a_small_head_next_to_a_large_one_and_floors_cancelled_blocks():
    B, L = 2, 9
    b = torch.randn(B * L, T.D, dtype=T.F64)
    b[:, :T.DH] *= 1e-3                                              # head 0 a thousand times smaller
    a = b.clone()
    a[3, 5] *= 1.01
    whole = ((a - b).abs().max() / b.abs().max()).item()
    assert T.block_err(a, b, T.blk_rows(B, L)) > 100 * whole
    z = torch.zeros(B * L, T.D, dtype=T.F64)
    assert T.block_err(z, z, T.blk_rows(B, L)) == 0.0 and T.block_err(z + 1e-30, z, T.blk_rows(B, L)) == float('inf')
    assert T.block_err(z + 1e-9, z, T.blk_rows(B, L), mag=z + 1.0) == pytest.approx(1e-9)          # cancelled: on the scale of the sum of |terms|
    assert T.block_err(a, b, T.blk_rows(B, L), mag=b.abs() * 31) == T.block_err(a, b, T.blk_rows(B, L))      # not cancelled: the plain measure
    assert T.block_err(a, b, T.blk_rows(B, L), mag=b.abs() * 33) < T.block_err(a, b, T.blk_rows(B, L)) / 30
    assert math.isnan(T.block_err(a * float('nan'), b, T.blk_rows(B, L)))


def test_only_blocks_of_samples_with_one_visible_key_are_measured_on_the_cancelled_scale():
    """Everywhere else the measure is max|a - b| / max|b| within the block, as it reads."""
    def cancelled_samples(b, mag, blocks, sample_of):
        den, m = blocks(b.double()).abs().amax(1), blocks(mag.double()).abs().amax(1)
        return {sample_of(i) for i in torch.nonzero(den < T.CANCELLED * m).flatten().tolist()}
    for fam, cases in (('self', T.SELF_CASES), ('cross', T.CROSS_CASES)):
        for c in cases:
            if 'gauss' not in c['kinds']:
                continue
            own = fam == 'self'
            B, Lq, Lk = c['B'], c['L'] if own else c['Lq'], c['L'] if own else c['Lk']
            fwd, bwd, mag = (T.self_reference if own else T.cross_reference)(c['name'], 'gauss', K[fam, c['name']])
            kpm = T.make_kpm(c['kpm'], B, Lk, Lk)
            single = {b for b in range(B) if (Lk if kpm is None else int((~kpm[b]).sum())) == 1}
            got = cancelled_samples(fwd['lse'], fwd['mag_lse'], T.blk_lse(B, Lq), lambda i: i // T.H)
            got |= cancelled_samples(bwd['dxpart'], mag['dxpart'], T.blk_parts(B, Lq), lambda i: i % B)
            if own:
                got |= cancelled_samples(bwd['dqkv'], mag['dqkv'], T.blk_rows(B, Lq, 3), lambda i: i // (3 * T.H))
            else:
                got |= cancelled_samples(bwd['dq'], mag['dq'], T.blk_rows(B, Lq), lambda i: i // T.H)
                got |= cancelled_samples(bwd['dk'], mag['dk'], T.blk_rows(B, Lk), lambda i: i // T.H)
            assert got <= single, f'{fam} {c["name"]}: samples {sorted(got - single)} have cancelled blocks and more than one visible key'


# ------------------------------------------------------------------------------------------------------------------------ the tests must be able to fail
def _apart(wrong, right, blocks, key, what):
    e = T.block_err(wrong, right, blocks)
    assert e >= FACTOR * T.bound(key), f'{what}: moves {key} by {e:.3e} < {FACTOR:.0f} x {T.bound(key):.1e}'


def test_sensitive_to_two_heads_swapped_in_a_ypart_plane():
    c = T.SELF_BY_NAME['L9-B3-ragged']
    y = T.self_reference(c['name'], 'gauss', K['self', c['name']])[0]['ypart']
    wrong = y.clone()
    wrong[[2, 3]] = y[[3, 2]]
    _apart(wrong, y, T.blk_parts(c['B'], c['L']), 'self_ypart', 'heads 2 and 3 swapped')
    yu = T.self_reference('U-L16-B3-pow2', 'uniform', K['self', 'U-L16-B3-pow2'])[0]['ypart']
    assert not torch.equal(yu[[3, 2]], yu[[2, 3]])                   # ... and breaks equality in the exact tier


@pytest.mark.parametrize('what', ['mask shifted by one', 'key L-1 treated as padding', 'scale applied twice'])
def test_sensitive_to_a_wrong_key_mask_or_scale(what):
    for fam, c in (('self', T.SELF_BY_NAME['L16-B3-ragged-pitched']), ('cross', T.CROSS_BY_NAME['Lq9-Lk17-B3-ragged-pitched'])):
        own = fam == 'self'
        t = (T.self_inputs if own else T.cross_inputs)(c, 'gauss')
        right = (T.self_reference if own else T.cross_reference)(c['name'], 'gauss', K[fam, c['name']])[0]
        kpm, scale = t['kpm'], T.SCALE
        if what == 'mask shifted by one':
            kpm = kpm.roll(1, 1)
        elif what == 'key L-1 treated as padding':
            kpm = kpm.clone()
            kpm[:, -1] = True
        else:
            scale = T.SCALE * T.SCALE
        wrong = (T.self_fwd_ref if own else T.cross_fwd_ref)(t, c, scale=scale, kpm=kpm)
        Lq = c['L'] if own else c['Lq']
        _apart(wrong['o'], right['o'], T.blk_rows(c['B'], Lq), fam + '_o', what)
        _apart(wrong['lse'], right['lse'], T.blk_lse(c['B'], Lq), fam + '_lse', what)
        _apart(wrong['ypart'], right['ypart'], T.blk_parts(c['B'], Lq), fam + '_ypart', what)
    # the exact tier: one key more or fewer changes o
    cu = T.SELF_BY_NAME['U-L16-B3-pow2']
    tu = T.self_inputs(cu, 'uniform')
    assert not torch.equal(T.self_fwd_ref(tu, cu, kpm=tu['kpm'].roll(1, 1))['o'], T.self_reference(cu['name'], 'uniform', K['self', cu['name']])[0]['o'])


def test_sensitive_to_a_hidden_slice_shifted_by_32_columns():
    c = T.FFN_BY_NAME['M70-F320-pitched']
    for kind in ('gauss', 'dyadic'):
        right = T.ffn_reference(c['name'], kind, K['ffn', c['name']])[0]['ypart']
        wrong = T.ffn_fwd_ref(T.ffn_inputs(c, kind), c, slice_shift=32)['ypart']
        if kind == 'gauss':
            _apart(wrong, right, T.blk_slices(c['M'], c['F']), 'ffn_ypart', 'slice 0 shifted by 32')
        assert not torch.equal(wrong, right) and torch.equal(wrong[1:], right[1:])


def test_sensitive_to_dk_and_dv_exchanged():
    c = T.CROSS_BY_NAME['Lq9-Lk17-B3-ragged-pitched']
    bwd = T.cross_reference(c['name'], 'gauss', K['cross', c['name']])[1]
    _apart(bwd['dv'], bwd['dk'], T.blk_rows(c['B'], c['Lk']), 'cross_dk', 'dv where dk belongs')
    _apart(bwd['dk'], bwd['dv'], T.blk_rows(c['B'], c['Lk']), 'cross_dv', 'dk where dv belongs')
    cu = T.CROSS_BY_NAME['U-Lq9-Lk33-B3-pow2-pitched']
    bu = T.cross_reference(cu['name'], 'uniform', K['cross', cu['name']])[1]
    assert not torch.equal(bu['dk'], bu['dv'])


def test_sensitive_to_a_missing_one_over_keep():
    c = T.FFN_BY_NAME['M70-F128-drop']
    t, k = T.ffn_inputs(c, 'gauss'), K['ffn', c['name']]
    fwd, bwd = T.ffn_reference(c['name'], 'gauss', k)
    wrong_b = T.ffn_bwd_ref(t, fwd, c, keep_scale=1.0)
    _apart(wrong_b['dh'], bwd['dh'], T.blk_tiles(c['M'], c['F']), 'ffn_dh', '1 / keep missing')
    _apart(wrong_b['dxpart'], bwd['dxpart'], T.blk_slices(c['M'], c['F']), 'ffn_dxpart', '1 / keep missing')
    wrong_f = T.ffn_fwd_ref(t, c, (T.ffn_drop(c, MASKS, k) > 0).double())
    _apart(wrong_f['h'], fwd['h'], T.blk_tiles(c['M'], c['F']), 'ffn_h', '1 / keep missing')
    for fam, c in (('self', T.SELF_BY_NAME['L9-B3-ragged-drop']), ('cross', T.CROSS_BY_NAME['Lq9-Lk33-B3-ragged-drop'])):
        own = fam == 'self'
        t, k = (T.self_inputs if own else T.cross_inputs)(c, 'gauss'), K[fam, c['name']]
        fwd, bwd, _ = (T.self_reference if own else T.cross_reference)(c['name'], 'gauss', k)
        drop01 = ((T.self_drop if own else T.cross_drop)(c, MASKS, k) > 0).double()
        Lq = c['L'] if own else c['Lq']
        _apart((T.self_fwd_ref if own else T.cross_fwd_ref)(t, c, drop01)['o'], fwd['o'], T.blk_rows(c['B'], Lq), fam + '_o', '1 / keep missing')
        wrong_b = (T.self_bwd_ref if own else T.cross_bwd_ref)(t, fwd, c, drop01)[0]
        _apart(wrong_b['dxpart'], bwd['dxpart'], T.blk_parts(c['B'], Lq), fam + '_dxpart', '1 / keep missing')


# ------------------------------------------------------------------------------------------------------------------------ against the pinned oracle
def _seq_first(t, B, L):
    return t.reshape(B, L, T.D).permute(1, 0, 2)


def test_self_attention_reference_is_detr_ref_mha():
    c = T.SELF_BY_NAME['L9-B3-ragged']
    t = T.self_inputs(c, 'gauss')
    fwd, bwd, _ = T.self_reference(c['name'], 'gauss', K['self', c['name']])
    b_out = torch.randn(T.D, dtype=T.F64, generator=torch.Generator().manual_seed(5))
    sd = {'in_proj_weight': t['w_in'].double().requires_grad_(True), 'in_proj_bias': t['b_in'].double(), 'out_proj.weight': t['w_out'].double(), 'out_proj.bias': b_out}
    x = t['x'].double().requires_grad_(True)
    xs = _seq_first(x, c['B'], c['L'])
    y = detr_ref.mha(sd, '', xs, xs, xs, T.H, t['kpm']).permute(1, 0, 2).reshape(-1, T.D)
    full = T.self_fwd_ref(t, c, scale=EXACT_SCALE)
    assert DC.rel_err(full['ypart'].sum(0) + b_out, y) < 1e-12 and DC.rel_err(fwd['ypart'].sum(0) + b_out, y) < 1e-7
    # the backward: dx = sum of the heads' dxpart (dr = gradient of y before the bias), on the unrounded saved tensors and on the rounded ones
    (dx,) = torch.autograd.grad(y, x, t['dr'].double())
    assert DC.rel_err(T.self_bwd_ref(t, dict(full, unrounded=True), c, scale=EXACT_SCALE)[0]['dxpart'].sum(0), dx) < 1e-11
    assert DC.rel_err(bwd['dxpart'].sum(0), dx) < 1e-5


def test_cross_attention_reference_is_detr_ref_mha():
    c = T.CROSS_BY_NAME['Lq9-Lk17-B3-ragged-pitched']
    t = T.cross_inputs(c, 'gauss')
    fwd, _, _ = T.cross_reference(c['name'], 'gauss', K['cross', c['name']])
    g = torch.Generator().manual_seed(6)
    mem, w_kv, b_kv = torch.randn(c['B'] * c['Lk'], T.D, dtype=T.F64, generator=g), torch.randn(2 * T.D, T.D, dtype=T.F64, generator=g) / 16, torch.randn(2 * T.D, dtype=T.F64, generator=g)
    kv = mem @ w_kv.t() + b_kv
    t2 = dict(t, k=kv[:, :T.D], v=kv[:, T.D:])
    b_out = torch.randn(T.D, dtype=T.F64, generator=g)
    sd = {'in_proj_weight': torch.cat([t['w_q'].double(), w_kv]), 'in_proj_bias': torch.cat([t['b_q'].double(), b_kv]), 'out_proj.weight': t['w_out'].double(), 'out_proj.bias': b_out}
    ms = _seq_first(mem, c['B'], c['Lk'])
    xq = t['x'].double().requires_grad_(True)
    y = detr_ref.mha(sd, '', _seq_first(xq, c['B'], c['Lq']), ms, ms, T.H, t['kpm']).permute(1, 0, 2).reshape(-1, T.D)
    full = T.cross_fwd_ref(t2, c, scale=EXACT_SCALE)
    assert DC.rel_err(full['ypart'].sum(0) + b_out, y) < 1e-12
    (dx,) = torch.autograd.grad(y, xq, t['dr'].double())
    assert DC.rel_err(T.cross_bwd_ref(t2, dict(full, unrounded=True), c, scale=EXACT_SCALE)[0]['dxpart'].sum(0), dx) < 1e-11
    assert fwd['ypart'].shape == (T.H, c['B'] * c['Lq'], T.D)


def test_feed_forward_reference_is_detr_ref_ffn():
    c = T.FFN_BY_NAME['M70-F320-pitched']
    t = T.ffn_inputs(c, 'gauss')
    fwd, bwd = T.ffn_reference(c['name'], 'gauss', K['ffn', c['name']])
    b2 = torch.randn(T.D, dtype=T.F64, generator=torch.Generator().manual_seed(7))
    sd = {'linear1.weight': t['w1'].double(), 'linear1.bias': t['b1'].double(), 'linear2.weight': t['w2'].double(), 'linear2.bias': b2}
    x = t['x'].double().requires_grad_(True)
    y = detr_ref._ffn(sd, '', x)
    assert DC.rel_err(fwd['ypart'].sum(0) + b2, y) < 1e-12
    (dx,) = torch.autograd.grad(y, x, t['dy'].double())
    assert DC.rel_err(bwd['dxpart'].sum(0), dx) < 1e-12              # the mask is read off h: rounding h to float32 does not move it


def test_a_fully_masked_sample_is_nan_in_the_reference_and_nowhere_else():
    for fam, c in (('self', T.SELF_MASKED), ('cross', T.CROSS_MASKED)):
        fwd = (T.self_reference if fam == 'self' else T.cross_reference)(c['name'], 'gauss', K[fam, c['name']])[0]
        Lq = c['L'] if fam == 'self' else c['Lq']
        rows = torch.zeros(c['B'] * Lq, dtype=torch.bool)
        rows[Lq:2 * Lq] = True
        assert torch.equal(fwd['o'].isnan().all(1), rows) and torch.equal(fwd['o'].isnan().any(1), rows)
        assert torch.equal(fwd['ypart'].isnan().all(2), rows.expand(T.H, -1)) and torch.equal(fwd['ypart'].isnan().any(2), rows.expand(T.H, -1))
