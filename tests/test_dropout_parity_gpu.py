"""Exact-mask fp64 parity of every dropout site of the training path.  The kernels' dropout generator is a pure function of (seed, element index), so
oracle/dropout_ref.py rebuilds every mask on the host from the seeds a launch was given (host half: hip.core.next_seed(), recorded here; device half:
the word hip.core.iter_seed() holds, redrawn by core.reseed() so that it is non-zero) and the fp64 reference multiplies by it: a backward that
regenerates another mask than its forward, a missing 1 / (1 - p), another site's p or seed, a dropped device word or a truncated seed sum all show up
as O(1) errors (tests/test_dropout_ref_cpu.py proves each of them moves the reference by > 100 x the tolerance).  Tolerances: the matching
dropout-off tests' own (dropout_common.TOL_*), unchanged -- the mask is an exact 0 / constant factor.  Every case prints its figures before it asserts."""
import contextlib
import copy
import ctypes

import pytest
import torch

import dropout_common as C

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def recorded_seeds(core):
    """The host halves of the dropout seeds drawn inside the block, in draw order."""
    real, seeds = core.next_seed, []

    def spy():
        s = real()
        seeds.append(s)
        return s
    core.next_seed = spy
    try:
        yield seeds
    finally:
        core.next_seed = real


def fresh_device_word(core, dev, case):
    """Redraws the device half of the seed (non-zero: its addition and the 64-bit carry are exercised) and pins both halves to the case: torch's
    generators seed the redraw and the upper half of next_seed(), the launch counter its lower half -- the masks, and with them which hidden units sit
    near the relu's kink, are the same in every run and whichever tests ran before."""
    torch.manual_seed(0xD20 + case)
    core._seed_counter[0] = 0x5EED + 64 * case
    core.reseed(dev)
    word = core.iter_seed().item()
    assert word != 0
    return C.Masks(word)


class Figures(object):
    """Collects (name, error, tolerance), prints each, asserts them together at the end of a case."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def add(self, name, a, b, tol):
        self.rows.append((name, C.rel_err(a, b), tol))

    def check(self):
        for name, e, tol in self.rows:
            print(f'[dropout parity] {self.case}: {name} rel err {e:.3e} (tol {tol:.1e})')
        bad = [f'{name}: {e:.3e} > {tol:.1e}' for name, e, tol in self.rows if not e <= tol]
        assert not bad, f'{self.case}: ' + '; '.join(bad)


# ------------------------------------------------------------------------------------------ a. attention core
ATTN_SHAPES = [(2, 2, 9, 9, 32),        # attn_fwd_kernel<1>, attn_bwd_kernel<1>
               (2, 2, 10, 24, 32),      # fwd <2>, attn_bwd_lds_kernel
               (1, 2, 16, 40, 32),      # fwd <4>, lds backward with a ragged key tile
               (2, 2, 64, 64, 32),      # attn_fwd_wide_kernel, lds backward at its full size
               (1, 2, 9, 100, 32),      # fwd <8>, bwd <8>
               (1, 2, 33, 200, 32),     # <16>, ragged query tile
               (1, 1, 20, 300, 32),     # attn_fwd_long_kernel, the chunk loop of attn_bwd_dq with a ragged second chunk
               (2, 2, 9, 40, 64),       # wide head, DHC 2 backward
               (1, 2, 70, 130, 64),     # wide forward: two query blocks, three key chunks
               (1, 2, 9, 9, 96)]        # DHC 3
ATTN_CASES = [s + (0.1,) for s in ATTN_SHAPES] + [s + (0.5,) for s in ATTN_SHAPES[:3]]


@pytest.mark.parametrize('B,H,Lq,Lk,dh,p', ATTN_CASES)
def test_attention_dropout_exact_mask_vs_fp64(dev, B, H, Lq, Lk, dh, p):
    """hip.attention.attention with dropout on the probabilities, every forward / backward kernel path (ATTN_SHAPES), ragged key-padding masks: o, dq, dk
    and dv against fp64 with the replica's mask at element ((b*H + h)*Lq + q)*Lk + key.
    Largest measured errors (MI355X): o 7.6e-7, gradients 7.0e-7 (tolerances 5e-6 / 2e-5)."""
    from layoutdetr_amd.hip import attention, core
    q, k, v, go, kpm = C.attention_inputs(B, H, Lq, Lk, dh)
    masks = fresh_device_word(core, dev, ATTN_CASES.index((B, H, Lq, Lk, dh, p)))
    qg, kg, vg = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
    with recorded_seeds(core) as seeds:
        og = attention.attention(qg, kg, vg, kpm.to(dev), B, H, Lq, Lk, p)
    og.backward(go.to(dev))
    assert len(seeds) == 1
    o, dq, dk, dv = C.attention_ref(q, k, v, go, kpm, B, H, Lq, Lk, dh, masks.attention(seeds[0], p, B, H, Lq, Lk))
    f = Figures(f'attention {(B, H, Lq, Lk, dh)} p={p}')
    f.add('o', og, o, C.TOL_ATTN['o']); f.add('dq', qg.grad, dq, C.TOL_ATTN['grad'])
    f.add('dk', kg.grad, dk, C.TOL_ATTN['grad']); f.add('dv', vg.grad, dv, C.TOL_ATTN['grad'])
    f.check()


@pytest.mark.parametrize('B,H,L,dh', [(2, 2, 17, 32), (1, 2, 40, 64)])
def test_attention_packed_causal_dropout_exact_mask_vs_fp64(dev, B, H, L, dh):
    """_AttnPackedFn on a packed [B*L, 3d] projection (row pitch 3d, not d) with the causal mask, a ragged key-padding mask and p = 0.1: o and the
    packed gradient's dq | dk | dv blocks against fp64 with the replica's mask.
    Largest measured errors (MI355X): o 3.9e-7, gradients 8.3e-7 (tolerances 5e-6 / 2e-5)."""
    from layoutdetr_amd.hip import attention, core
    p, d = 0.1, H * dh
    q, k, v, go, kpm = C.attention_inputs(B, H, L, L, dh)
    masks = fresh_device_word(core, dev, 20 + L)
    qkv = torch.cat([q, k, v], 1).to(dev).requires_grad_(True)
    with recorded_seeds(core) as seeds:
        og = attention._AttnPackedFn.apply(qkv, None, attention.kpm_u8(kpm.to(dev)), B, H, L, p, True)
    og.backward(go.to(dev))
    assert len(seeds) == 1
    o, dq, dk, dv = C.attention_ref(q, k, v, go, kpm, B, H, L, L, dh, masks.attention(seeds[0], p, B, H, L, L), causal=True)
    f = Figures(f'packed causal attention {(B, H, L, dh)}')
    f.add('o', og, o, C.TOL_ATTN['o'])
    for name, ref, blk in (('dq', dq, 0), ('dk', dk, 1), ('dv', dv, 2)):
        f.add(name, qkv.grad[:, blk * d:(blk + 1) * d], ref, C.TOL_ATTN['grad'])
    f.check()


# ------------------------------------------------------------------------------------------ b. token stacks in train mode
@pytest.mark.parametrize('kind,B,L,S', [('enc', 3, 9, 0), ('enc', 2, 16, 0), ('enc', 1, 1, 0),
                                        ('dec', 3, 9, 37), ('dec', 2, 10, 64),      # the one-launch cross path
                                        ('dec', 2, 9, 80)])                         # the generic cross path onto ldetr_attention_* with grouped K / V pitches
def test_token_stack_node_train_mode_vs_fp64_oracle(dev, kind, B, L, S):
    """test_token_stack_node_vs_fp64_oracle's set-up (2 layers, d 256, 8 heads, the stack node through forward2d) in TRAIN mode with a different p at
    every dropout site of a layer (self-attention 0.15, cross-attention 0.25, residuals 0.1 / 0.2 / 0.3, hidden 0.35): output, dx, d memory and every
    parameter gradient against the fp64 oracle with the replica's masks (oracle/detr_ref.py's drop hook).  A lone stack draws, per layer: self-attention;
    for a decoder norm1, then cross-attention; norm_a, hidden, norm_b.
    Largest measured errors (MI355X): y 1.9e-7, gradients 7.8e-7 (tolerances 2e-5 / 5e-5)."""
    from layoutdetr_amd.hip import core
    from layoutdetr_amd.hip import stacks as hstacks
    mod = C.stack_module(kind)
    x, gy, kpm, mem_kpm, mem, pos = C.stack_inputs(kind, B, L, S)
    assert mod.training
    mod.to(dev)
    masks = fresh_device_word(core, dev, 30 + B * L + S)
    xg = x.to(dev).requires_grad_(True)
    assert hstacks.ENABLED
    n0 = hstacks.NODE_RUNS[0]
    with recorded_seeds(core) as seeds:
        if kind == 'enc':
            y = mod.forward2d(xg, B, L, kpm.to(dev), None)
        else:
            memg = mem.to(dev).requires_grad_(True)
            y = mod.forward2d(xg, memg, pos.to(dev).repeat(B, 1), B, L, S, kpm.to(dev), mem_kpm.to(dev))
    assert hstacks.NODE_RUNS[0] == n0 + 1, 'the stack did not take the stack node'
    (y * gy.to(dev)).sum().backward()
    yr, dxr, dmemr, gr = C.stack_ref(kind, mod, x, gy, kpm, mem_kpm, mem, pos, B, L, S, C.stack_drop(kind, seeds, masks, B, L, S))
    f = Figures(f'{kind} stack {(B, L, S)}')
    f.add('y', y, yr, C.TOL_STACK['y']); f.add('dx', xg.grad, dxr, C.TOL_STACK['grad'])
    if kind == 'dec':
        f.add('d memory', memg.grad, dmemr, C.TOL_STACK['grad'])
    named = dict(mod.named_parameters())
    assert set(gr) == set(named)
    for k_, g in gr.items():
        assert named[k_].grad is not None, k_
        f.add('d ' + k_, named[k_].grad, g, C.TOL_STACK['grad'])
    f.check()


# ------------------------------------------------------------------------------------------ c. the unfused sub-blocks
@pytest.mark.parametrize('rows,D,pos_rows', [(18, 256, 9), (5, 64, 0), (37, 768, 0)])
def test_add_layernorm_dropout_exact_mask_vs_fp64(dev, rows, D, pos_rows):
    """LayerNorm(x + dropout(r)) with p = 0.1, both directions: y, the second output y + pos, dx, dr, dgamma, dbeta against fp64 with the replica's mask
    at element row*D + col.
    Largest measured errors (MI355X): y 1.1e-7, gradients 1.8e-7 (tolerances 3e-6 / 1e-5)."""
    from layoutdetr_amd.hip import core, layernorm
    p = 0.1
    t = C.layernorm_inputs(rows, D, pos_rows)
    masks = fresh_device_word(core, dev, 40 + rows)
    xg, rg, gg, bg = [t[k].to(dev).requires_grad_(True) for k in ('x', 'r', 'gamma', 'beta')]
    with recorded_seeds(core) as seeds:
        out = layernorm.add_layernorm(xg, rg, gg, bg, 1e-5, p, pos=t['pos'].to(dev) if pos_rows else None)
    y, ypos = out if pos_rows else (out, None)
    loss = (y * t['gy'].to(dev)).sum()
    if pos_rows:
        loss = loss + (ypos * t['gp'].to(dev)).sum()
    loss.backward()
    assert len(seeds) == 1
    ref = C.layernorm_ref(t, masks.rows(seeds[0], p, rows, D))
    f = Figures(f'add_layernorm {(rows, D)}')
    f.add('y', y, ref['y'], C.TOL_LN['y'])
    if pos_rows:
        f.add('y + pos', ypos, ref['ypos'], C.TOL_LN['y'])
    for name, a in (('dx', xg.grad), ('dr', rg.grad), ('dgamma', gg.grad), ('dbeta', bg.grad)):
        f.add(name, a, ref[name], C.TOL_LN['grad'])
    f.check()


@pytest.mark.parametrize('M,F_', [(33, 64), (144, 2048)])
def test_ln_ffn_ln_fused_tail_dropout_exact_masks_vs_fp64(dev, M, F_):
    """hip.ffn.add_ln_ffn_add_ln with p_res = 0.1 at both residuals and p_h = 0.2 on the hidden activation against fp64 with the three masks (row*D + col,
    m*F + col, row*D + col; seeds drawn in that order): output, dx, dr and all parameter gradients -- exact parity next to the finite-difference check
    of test_ln_ffn_ln_fused_tail_train_mode_dropout_and_reproducibility.  Gradients in close_up_to_relu_flips' measure (share of entries off by more
    than 2e-5 of the maximum <= 3 %).
    Largest measured (MI355X): y 1.9e-7; share of entries off 0 for every gradient, largest entry error 3.3e-7."""
    from layoutdetr_amd.hip import core, ffn
    p_res, p_h = 0.1, 0.2
    mods, x, r, gy = C.ffn_modules(M, F_)
    l1, l2, lna, lnb = mods
    D = x.shape[1]
    masks = fresh_device_word(core, dev, 50 + M)
    gmods = [copy.deepcopy(m).to(dev) for m in mods]
    g1, g2, gna, gnb = gmods
    xg, rg = x.to(dev).requires_grad_(True), r.to(dev).requires_grad_(True)
    assert ffn.usable(xg, g1, g2)
    with recorded_seeds(core) as seeds:
        y = ffn.add_ln_ffn_add_ln(xg, rg, gna, p_res, g1, g2, gnb, p_h, p_res)
    (y * gy.to(dev)).sum().backward()
    assert len(seeds) == 3
    yr, dxr, drr, pgr = C.ffn_ref(mods, x, r, gy, masks.rows(seeds[0], p_res, M, D), masks.rows(seeds[1], p_h, M, F_), masks.rows(seeds[2], p_res, M, D))
    e_y = C.rel_err(y, yr)
    print(f'[dropout parity] ffn tail {(M, F_)}: y rel err {e_y:.3e} (tol {C.TOL_FFN["y"]:.1e})')
    bad = [] if e_y <= C.TOL_FFN['y'] else [f'y: {e_y:.3e}']
    names = ['dx', 'dr'] + [f'grad {type(m).__name__}{i}.{n}' for i, m in enumerate(gmods) for n, _ in m.named_parameters()]
    got = [xg.grad, rg.grad] + [p_.grad for m in gmods for p_ in m.parameters()]
    for name, a, b in zip(names, got, [dxr, drr] + pgr):
        share, worst = C.relu_flip_share(a, b, C.TOL_FFN['thresh'])
        print(f'[dropout parity] ffn tail {(M, F_)}: {name}: {share:.4f} of the entries off by more than {C.TOL_FFN["thresh"]:.0e}, max {worst:.2e}')
        if not share <= C.TOL_FFN['share']:
            bad.append(f'{name}: {share:.4f} of the entries off, max {worst:.2e}')
    assert not bad, '; '.join(bad)


@pytest.mark.parametrize('M,N,K,kind', [(18, 64, 256, 2),         # gemm_small_kernel (register-streaming 32 x 32 tiles)
                                        (520, 2048, 256, 1)])     # gemm_f32_kernel (LDS-tiled): 9 x 32 tiles of 64 x 64 are past the small-tile class (< 256 tiles)
def test_linear_relu_dropout_epilogue_exact_mask_vs_fp64(dev, M, N, K, kind):
    """linear(act=ACT_RELU, p_drop=0.25): the GEMM epilogue's dropout at element row*ldc + col on both engine kernels (the launched kind asserted through
    ldetr_engine_last_launch, so a policy change cannot silently drop a path): forward, dx, dW, db against fp64 with the replica's mask.
    Largest measured errors (MI355X): y 3.2e-7, gradients 3.6e-7 (tolerances 3e-6 / 5e-6)."""
    from layoutdetr_amd.hip import core, linear
    p = 0.25
    x, w, b, gy = C.linear_inputs(M, N, K)
    masks = fresh_device_word(core, dev, 60 + M)
    xg, wg, bg = [t.to(dev).requires_grad_(True) for t in (x, w, b)]
    with recorded_seeds(core) as seeds:
        y = linear.linear(xg, wg, bg, act=core.ACT_RELU, p_drop=p)
    info = (ctypes.c_int32 * 10)()
    core.check(core.lib().ldetr_engine_last_launch(info), 'engine_last_launch')
    assert info[0] == kind, f'launched {core.launched_kernel("gemm")}, expected engine kind {kind}'
    y.backward(gy.to(dev))
    assert len(seeds) == 1
    yr, dxr, dwr, dbr = C.linear_ref(x, w, b, gy, masks.rows(seeds[0], p, M, N, ld=y.stride(0)))
    f = Figures(f'linear {(M, N, K)} kind {kind}')
    f.add('y', y, yr, C.TOL_LINEAR['y']); f.add('dx', xg.grad, dxr, C.TOL_LINEAR['grad'])
    f.add('dW', wg.grad, dwr, C.TOL_LINEAR['grad']); f.add('db', bg.grad, dbr, C.TOL_LINEAR['grad'])
    f.check()


def test_mha_forward_same_qk_dropout_exact_mask_vs_fp64(dev):
    """mha_forward(same_qk=True, qk_pos=...) at B = 2, L = 64, d = 256, H = 8, p = 0.1 -- the packed q | k projection with a separate v (the 64-token
    encoder's self-attention block) under dropout -- against oracle/detr_ref.mha with the replica's mask: output, dx and every parameter gradient.
    Tolerance: dropout_common.TOL_MHA (the stages' own bounds added up).
    Largest measured errors (MI355X): y 3.8e-7, gradients 5.1e-7 (tolerances 2e-5 / 5e-5)."""
    from layoutdetr_amd.hip import attention, core
    B, L, d, H, p = 2, 64, 256, 8, 0.1
    sd, x, pos, gy, kpm = C.mha_inputs(B, L, d)
    masks = fresh_device_word(core, dev, 70)
    par = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}
    xg = x.to(dev).requires_grad_(True)
    with recorded_seeds(core) as seeds:
        y = attention.mha_forward(xg, xg, xg, par['in_proj_weight'], par['in_proj_bias'], par['out_proj.weight'], par['out_proj.bias'], H, B, L, L,
                                  key_padding_mask=kpm.to(dev), p_drop=p, same_qk=True, qk_pos=pos.to(dev).repeat(B, 1))
    (y * gy.to(dev)).sum().backward()
    assert len(seeds) == 1
    yr, dxr, gr = C.mha_ref(sd, x, pos, gy, kpm, B, L, d, H, masks.attention(seeds[0], p, B, H, L, L))
    f = Figures('mha_forward same_qk')
    f.add('y', y, yr, C.TOL_MHA['y']); f.add('dx', xg.grad, dxr, C.TOL_MHA['grad'])
    for k_, g in gr.items():
        f.add('d ' + k_, par[k_].grad, g, C.TOL_MHA['grad'])
    f.check()
