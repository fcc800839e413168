"""The numpy replica of the kernels' dropout generator (oracle/dropout_ref.py) against vectors computed from a C transcription of
csrc/ldetr_common.hpp, the oracle's explicit-mask hook, and -- for one case of every family of tests/test_dropout_parity_gpu.py -- the proof that the
family's tolerance separates the right mask convention from a wrong one: the fp64 reference evaluated with a deliberately wrong convention differs
from the right one by at least 100 x the tolerance, in the same measure.  No GPU needed."""
import numpy as np
import pytest
import torch

import dropout_common as C
from oracle import detr_ref
from oracle import dropout_ref as DR

IDX = np.array([0, 1, 2, 3, 2 ** 32 + 7], dtype=np.uint64)
BITS = {0x5EED: [4173243739, 1263926963, 4066965651, 535570341, 629636753],
        0x0000002A9E3779B1: [4000394679, 3543479278, 2438662262, 3054817887, 1059479764],
        0x15: [1097281630, 2823433442, 1153648462, 2643415543, 1172717808]}
KEPT = {0x5EED: 900249, 0x0000002A9E3779B1: 900203}

# host halves as hip.core.next_seed() forms them, and a device word as .item() returns it (signed; its sum with a host half carries out of 64 bits)
HOST = [((0x1234 << 32) ^ (n * 0x9E3779B1)) & 0xFFFFFFFFFFFFFFFF for n in range(1, 16)]
WORD = -0x00000FFF89ABCDEF
FACTOR = 100.0


@pytest.mark.parametrize('seed', sorted(BITS))
def test_rng_bits_pinned_vectors(seed):
    out = DR.rng_bits(seed, IDX)
    assert out.dtype == np.uint32 and out.tolist() == BITS[seed]
    assert DR.rng_bits(seed + (1 << 64), IDX).tolist() == BITS[seed], 'the seed is taken mod 2^64'


@pytest.mark.parametrize('seed', sorted(KEPT))
def test_keep_count_over_a_million_elements(seed):
    k = DR.keep(seed, np.arange(10 ** 6), 0.1)
    assert k.dtype == np.bool_ and int(k.sum()) == KEPT[seed]


def test_keep_compares_in_float32_and_scales_by_the_rounded_p():
    bits = DR.rng_bits(0x5EED, np.arange(4096, dtype=np.uint64))
    u = (bits >> 8).astype(np.float64) / 2.0 ** 24
    for p in (0.1, 0.25, 0.5):
        assert np.array_equal(DR.keep(0x5EED, np.arange(4096), p), u >= float(np.float32(p)))
        assert DR.keep_scale(p) == 1.0 / (1.0 - float(np.float32(p)))
    s = DR.scale(0x5EED, np.arange(4096, dtype=np.uint64).reshape(64, 64), 0.1)
    assert s.shape == (64, 64) and set(np.unique(s).tolist()) == {0.0, DR.keep_scale(0.1)}


def test_total_seed_is_the_sum_mod_2_64():
    assert DR.total_seed(2 ** 64 - 1, 2) == 1
    assert DR.total_seed(5, -1) == 4                                   # the device word as a signed int64
    assert DR.total_seed(HOST[0], WORD) == (HOST[0] + (WORD & 0xFFFFFFFFFFFFFFFF)) % 2 ** 64
    assert (HOST[0] & 0xFFFFFFFF) + (WORD & 0xFFFFFFFF) >= 2 ** 32 and HOST[0] + (WORD & 0xFFFFFFFFFFFFFFFF) >= 2 ** 64, 'this pair carries in both halves'


def test_index_builders():
    B, H, Lq, Lk = 3, 2, 5, 7
    a = DR.attention_index(B, H, Lq, Lk)
    assert a.shape == (B, H, Lq, Lk) and a.dtype == np.uint64
    assert int(a[2, 1, 4, 6]) == ((2 * H + 1) * Lq + 4) * Lk + 6 and int(a[1, 0, 0, 3]) == ((1 * H) * Lq) * Lk + 3
    assert np.array_equal(a.reshape(-1), np.arange(B * H * Lq * Lk, dtype=np.uint64))
    r = DR.rows_index(4, 6)
    assert int(r[3, 5]) == 3 * 6 + 5 and np.array_equal(r.reshape(-1), np.arange(24, dtype=np.uint64))
    assert int(DR.rows_index(4, 6, 10)[3, 5]) == 35
    assert int(DR.rows_index(3, 4, 2 ** 31)[2, 3]) == 2 ** 32 + 3     # past 2^32: no 32-bit wrap in the index
    seed = DR.total_seed(HOST[1], WORD)
    assert np.array_equal(DR.attention_scale(seed, 0.1, B, H, Lq, Lk), DR.scale(seed, a, 0.1))
    assert np.array_equal(DR.layernorm_scale(seed, 0.1, 4, 6), DR.scale(seed, r, 0.1)) and np.array_equal(DR.hidden_scale(seed, 0.2, 4, 6), DR.scale(seed, r, 0.2))
    assert np.array_equal(DR.gemm_scale(seed, 0.25, 4, 6, 10), DR.scale(seed, DR.rows_index(4, 6, 10), 0.25))


def test_oracle_drop_hook_default_is_the_identity_and_sites_are_named():
    """drop=None leaves the oracle bit for bit as it was; an identity hook gives the same values and sees every site of a layer once, in order."""
    torch.manual_seed(5)
    d, H, B, L, S = 32, 4, 2, 5, 6
    g = lambda *s: torch.randn(*s)
    sd = {}
    for a in ('self_attn.', 'multihead_attn.'):
        sd.update({a + 'in_proj_weight': g(3 * d, d) * 0.2, a + 'in_proj_bias': g(3 * d) * 0.1, a + 'out_proj.weight': g(d, d) * 0.2, a + 'out_proj.bias': g(d) * 0.1})
    sd.update({'linear1.weight': g(64, d) * 0.2, 'linear1.bias': g(64) * 0.1, 'linear2.weight': g(d, 64) * 0.2, 'linear2.bias': g(d) * 0.1})
    for n in ('norm1.', 'norm2.', 'norm3.'):
        sd.update({n + 'weight': torch.rand(d) + 0.5, n + 'bias': g(d) * 0.1})
    sd = {'layers.0.' + k: v for k, v in sd.items()}
    x, mem, pos = g(L, B, d), g(S, B, d), g(S, B, d)
    kpm, mkpm = C.ragged_kpm(B, L), C.ragged_kpm(B, S)
    seen = []

    def ident(site, t):
        seen.append((site, tuple(t.shape)))
        return t
    e0 = detr_ref.torch_encoder(sd, '', x, H, kpm)
    assert torch.equal(detr_ref.torch_encoder(sd, '', x, H, kpm, ident), e0)
    assert seen == [('layers.0.attn', (B * H, L, L)), ('layers.0.res1', (L, B, d)), ('layers.0.hidden', (L, B, 64)), ('layers.0.res2', (L, B, d))]
    seen.clear()
    d0 = detr_ref.decoder_layer(sd, 'layers.0.', x, mem, H, kpm, mkpm, pos)
    assert torch.equal(detr_ref.decoder_layer(sd, 'layers.0.', x, mem, H, kpm, mkpm, pos, ident), d0)
    assert [s for s, _ in seen] == ['layers.0.' + p for p in ('attn', 'res1', 'cross', 'res2', 'hidden', 'res3')]
    assert seen[2][1] == (B * H, L, S)
    zero = detr_ref.encoder_layer(sd, 'layers.0.', x, H, kpm, None, lambda site, t: t * 0)      # every branch dropped: norm2(norm1(x))
    assert torch.allclose(zero, detr_ref._ln(sd, 'layers.0.norm2.', detr_ref._ln(sd, 'layers.0.norm1.', x)))


# ------------------------------------------------------------------------------------------ the tests must be able to fail
RIGHT = C.Masks(WORD)
WRONG_SEED = {'seed + 1': C.Masks(WORD, seed_shift=1), 'device word dropped': C.Masks(WORD, use_device_word=False)}
WRONG_ATTN = dict(WRONG_SEED, **{'q and key swapped': C.Masks(WORD, swap_qk=True), 'h*B + b for b*H + h': C.Masks(WORD, swap_bh=True)})


def _assert_apart(wrong, right, tol, what):
    e = C.rel_err(wrong, right)
    assert e >= FACTOR * tol, f'{what}: the wrong convention moves it by {e:.3e} < {FACTOR:.0f} x {tol:.1e}'


@pytest.mark.parametrize('wrong', sorted(WRONG_ATTN))
def test_attention_tolerance_rejects_wrong_convention(wrong):
    B, H, Lq, Lk, dh, p = 2, 2, 9, 9, 32, 0.1
    q, k, v, go, kpm = C.attention_inputs(B, H, Lq, Lk, dh)
    ref = C.attention_ref(q, k, v, go, kpm, B, H, Lq, Lk, dh, RIGHT.attention(HOST[0], p, B, H, Lq, Lk))
    bad = C.attention_ref(q, k, v, go, kpm, B, H, Lq, Lk, dh, WRONG_ATTN[wrong].attention(HOST[0], p, B, H, Lq, Lk))
    for name, a, b, tol in zip(('o', 'dq', 'dk', 'dv'), bad, ref, (C.TOL_ATTN['o'],) + (C.TOL_ATTN['grad'],) * 3):
        _assert_apart(a, b, tol, f'{wrong}: {name}')


@pytest.fixture(scope='module')
def stack_case():
    kind, B, L, S = 'dec', 2, 10, 64
    mod = C.stack_module(kind)
    inp = C.stack_inputs(kind, B, L, S)
    seeds = HOST[:12]
    ref = C.stack_ref(kind, mod, *inp, B, L, S, C.stack_drop(kind, seeds, RIGHT, B, L, S))
    return kind, B, L, S, mod, inp, seeds, ref


@pytest.mark.parametrize('wrong', sorted(WRONG_ATTN) + ["hidden's p at res2"])
def test_stack_tolerance_rejects_wrong_convention(stack_case, wrong):
    """Output, dx, d memory and every parameter gradient move by >= 100 x the tolerance -- except the closing norm's bias, whose gradient is the column
    sum of the output gradient whatever the masks are."""
    kind, B, L, S, mod, inp, seeds, ref = stack_case
    if wrong in WRONG_ATTN:
        drop = C.stack_drop(kind, seeds, WRONG_ATTN[wrong], B, L, S)
    else:
        drop = C.stack_drop(kind, seeds, RIGHT, B, L, S, p_of=dict(C.STACK_P, res2=C.STACK_P['hidden']))
    bad = C.stack_ref(kind, mod, *inp, B, L, S, drop)
    _assert_apart(bad[0], ref[0], C.TOL_STACK['y'], f'{wrong}: y')
    _assert_apart(bad[1], ref[1], C.TOL_STACK['grad'], f'{wrong}: dx')
    _assert_apart(bad[2], ref[2], C.TOL_STACK['grad'], f'{wrong}: d memory')
    assert torch.equal(bad[3]['norm.bias'], ref[3]['norm.bias'])
    for k_, g in ref[3].items():
        if k_ != 'norm.bias':
            _assert_apart(bad[3][k_], g, C.TOL_STACK['grad'], f'{wrong}: d {k_}')


@pytest.mark.parametrize('wrong', sorted(WRONG_SEED))
def test_layernorm_tolerance_rejects_wrong_convention(wrong):
    """(dbeta is the column sum of the output gradient: no mask reaches it.)"""
    rows, D, p = 18, 256, 0.1
    t = C.layernorm_inputs(rows, D, pos_rows=9)
    ref = C.layernorm_ref(t, RIGHT.rows(HOST[0], p, rows, D))
    bad = C.layernorm_ref(t, WRONG_SEED[wrong].rows(HOST[0], p, rows, D))
    for name in ('y', 'ypos', 'dx', 'dr', 'dgamma'):
        _assert_apart(bad[name], ref[name], C.TOL_LN['y' if name.startswith('y') else 'grad'], f'{wrong}: {name}')


@pytest.mark.parametrize('wrong', sorted(WRONG_SEED) + ["hidden's p at res2"])
def test_ffn_tail_tolerance_rejects_wrong_convention(wrong):
    """close_up_to_relu_flips would fail (more than 3 % of the entries off by more than 2e-5) and the largest entry is off by >= 100 x its threshold."""
    M, F_, p_res, p_h = 33, 64, 0.1, 0.2
    mods, x, r, gy = C.ffn_modules(M, F_)
    D = x.shape[1]

    def run(mk, p_b):
        return C.ffn_ref(mods, x, r, gy, mk.rows(HOST[0], p_res, M, D), mk.rows(HOST[1], p_h, M, F_), mk.rows(HOST[2], p_b, M, D))
    ref = run(RIGHT, p_res)
    bad = run(WRONG_SEED[wrong], p_res) if wrong in WRONG_SEED else run(RIGHT, p_h)
    _assert_apart(bad[0], ref[0], C.TOL_FFN['y'], f'{wrong}: y')
    names = ['dx', 'dr', 'dW1', 'db1', 'dW2', 'db2', 'dgamma_a', 'dbeta_a', 'dgamma_b']      # (dbeta_b: the column sum of gy)
    for name, a, b in zip(names, list(bad[1:3]) + bad[3], list(ref[1:3]) + ref[3]):
        share, worst = C.relu_flip_share(a, b, C.TOL_FFN['thresh'])
        assert share > C.TOL_FFN['share'] and worst >= FACTOR * C.TOL_FFN['thresh'], f'{wrong}: {name}: share {share:.4f}, max {worst:.2e}'


@pytest.mark.parametrize('wrong', sorted(WRONG_SEED) + ['row pitch N + 4'])
def test_linear_epilogue_tolerance_rejects_wrong_convention(wrong):
    M, N, K, p = 18, 64, 256, 0.25
    x, w, b, gy = C.linear_inputs(M, N, K)
    ref = C.linear_ref(x, w, b, gy, RIGHT.rows(HOST[0], p, M, N))
    bad_mask = WRONG_SEED[wrong].rows(HOST[0], p, M, N) if wrong in WRONG_SEED else RIGHT.rows(HOST[0], p, M, N, ld=N + 4)
    bad = C.linear_ref(x, w, b, gy, bad_mask)
    for name, a, b_, tol in zip(('y', 'dx', 'dW', 'db'), bad, ref, (C.TOL_LINEAR['y'],) + (C.TOL_LINEAR['grad'],) * 3):
        _assert_apart(a, b_, tol, f'{wrong}: {name}')


@pytest.mark.parametrize('M,N,K', [(18, 64, 256), (520, 2048, 256)])
def test_linear_inputs_keep_clear_of_the_relu_kink(M, N, K):
    """The GPU file's linear cases compare gradients entry by entry at 5e-6: no pre-activation may be close enough to 0 to flip under fp32 rounding."""
    x, w, b, _ = C.linear_inputs(M, N, K)
    pre = torch.nn.functional.linear(x.double(), w.double(), b.double())
    assert pre.abs().min().item() >= C.LINEAR_CLEARANCE
    assert (torch.nn.functional.linear(x, w, b).double() - pre).abs().max().item() <= C.LINEAR_CLEARANCE / 2


@pytest.mark.parametrize('wrong', sorted(WRONG_ATTN))
def test_mha_block_tolerance_rejects_wrong_convention(wrong):
    B, L, d, H, p = 2, 64, 256, 8, 0.1
    sd, x, pos, gy, kpm = C.mha_inputs(B, L, d)
    ref = C.mha_ref(sd, x, pos, gy, kpm, B, L, d, H, RIGHT.attention(HOST[0], p, B, H, L, L))
    bad = C.mha_ref(sd, x, pos, gy, kpm, B, L, d, H, WRONG_ATTN[wrong].attention(HOST[0], p, B, H, L, L))
    _assert_apart(bad[0], ref[0], C.TOL_MHA['y'], f'{wrong}: y')
    _assert_apart(bad[1], ref[1], C.TOL_MHA['grad'], f'{wrong}: dx')
    for k_ in ('in_proj_weight', 'in_proj_bias', 'out_proj.weight'):      # (out_proj.bias: the column sum of gy)
        _assert_apart(bad[2][k_], ref[2][k_], C.TOL_MHA['grad'], f'{wrong}: d {k_}')
