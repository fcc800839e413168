"""The encoder rider: two independent 64-token encoder stacks advanced in lock-step, one launch per step for both.

* the two-problem forward entries (ldetr_gemm_pair_fwd_f32, ldetr_attention_fwd_group_f32) against the single entries, bit for bit, outputs
  prefilled with NaN (guard rows and pitch gaps keep their bits);
* a 2-layer encoder pair with different weights at 64 / 128 rows, rider on against off: both memories and the trained half's input gradient
  bit-equal with dropout on, its parameter gradients (fp32 atomics) within 3x the off-against-off difference;
* one Gmain + Dmain iteration at B = 2 on 64x64 backgrounds, rider on against off from the same state and seeds: boxes and loss terms bit-equal,
  parameter gradients within 3x the off-against-off difference (both figures printed)."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def _padded(M, N, dev):
    """A NaN-filled [M + 3, N + 8] buffer and its [M, N] view (pitch N + 8: 16-byte aligned rows)."""
    buf = torch.full((M + 3, N + 8), NAN, device=dev)
    return buf, buf[:M, :N]


def _gemm_problem(M, N, K, kind, seed, dev):
    from layoutdetr_amd.hip import core
    g = torch.Generator().manual_seed(seed)
    A, W, b = torch.randn(M, K, generator=g).to(dev), (torch.randn(N, K, generator=g) / K ** 0.5).to(dev), torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev)
    if kind == 'bias':
        mk = lambda: core.epilogue(col_bias=b)
    elif kind == 'relu_drop':
        mk = lambda: core.epilogue(col_bias=b, act=core.ACT_RELU, p_drop=0.1, seed=0x1234 + seed)
    else:
        mk = lambda: core.epilogue(col_bias=b, residual=res)
    return dict(A=A, B=W, M=M, N=N, K=K, mk=mk, keep=(b, res))


@pytest.mark.parametrize('K,kinds', [(256, ('bias', 'relu_drop')), (256, ('relu_drop', 'residual')), (256, ('residual', 'bias')), (1024, ('bias', 'relu_drop'))])
def test_gemm_pair_fwd_bit_equal_to_single_launches(dev, K, kinds):
    """M = 35 and 70 (no multiple of the 32-row tile, different per half), N = 256.  K = 1024 on 16 / 24 tiles is the case small_plan_rule
    splits (tiles <= 128 and K >= 1024 -> K / 256 = 4 slices each, 4 x 24 <= 640): asserted from the launch record."""
    from layoutdetr_amd.hip import core
    core.iter_seed(dev).fill_(987654321)
    probs = [_gemm_problem(M, 256, K, kind, 10 * i + K, dev) for i, (M, kind) in enumerate(zip((35, 70), kinds))]
    single, paired = [], []
    for p in probs:
        buf, view = _padded(p['M'], p['N'], dev)
        core.gemm(p['A'], p['B'], 0, 0, p['M'], p['N'], p['K'], out=view, ep=p['mk']())
        single.append(buf)
    eps = [p['mk']() for p in probs]
    for p, ep in zip(probs, eps):
        buf, view = _padded(p['M'], p['N'], dev)
        p['out'], p['ep'], p['ta'], p['tb'] = view, ep, 0, 0
        paired.append(buf)
    descs = [core.gemm_desc(p['A'], p['B'], 0, 0, p['M'], p['N'], p['K'], p['out'], p['ep']) for p in probs]
    rc = core.lib().ldetr_gemm_pair_fwd_f32(ctypes.byref(descs[0]), ctypes.byref(descs[1]), core.stream())
    assert rc == 0, 'the two problems must go out as one launch'
    info = (ctypes.c_int32 * 10)()
    core.check(core.lib().ldetr_engine_last_launch(info), 'engine_last_launch')
    assert info[0] == 3, 'gemm_small_pair_kernel'
    sk0, sk1 = info[7] // 256, info[7] % 256
    if K >= 1024:
        assert sk0 > 1 and sk1 > 1, (sk0, sk1)
    else:
        assert (sk0, sk1) == (1, 1)
    torch.cuda.synchronize()
    for s, q, p in zip(single, paired, probs):
        assert not torch.isnan(s[:p['M'], :p['N']]).any()
        assert torch.equal(bits(s), bits(q))


def _attn_problem(B, L, seed, dev):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * L, 768, generator=g).to(dev)
    kpm = torch.zeros(B, L, dtype=torch.uint8)
    kpm[-1, L - 3:] = 1
    return dict(qkv=qkv, kpm=kpm.to(dev), B=B, L=L, seed=0xABC0 + seed)


def _attn_args(p, out, lse, dev):
    from layoutdetr_amd.hip import attention, core
    q, k, v = p['qkv'][:, :256], p['qkv'][:, 256:512], p['qkv'][:, 512:]
    a = attention._fwd_args(q, k, v, p['kpm'], out, lse, p['B'], 8, p['L'], p['L'], 32, 32 ** -0.5, 0.1, p['seed'], 0)
    assert (a.ldq, a.ldk, a.ldv) == (768, 768, 768) and a.seed_ptr == core.iter_seed(dev).data_ptr()
    return a


@pytest.mark.parametrize('L', [35, 64])
def test_attention_group_bit_equal_to_single_launches(dev, L):
    """One and two samples of a 5x7 map (35 / 70 rows; Lq < 48: attn_fwd_kernel) and of an 8x8 map (the 64-token encoders: attn_fwd_wide_kernel),
    8 heads x 32, key padding, dropout 0.1 with a seed per problem."""
    from layoutdetr_amd import _lib
    from layoutdetr_amd.hip import core
    core.iter_seed(dev).fill_(13579)
    probs = [_attn_problem(1, L, 1, dev), _attn_problem(2, L, 2, dev)]
    outs = []
    for n in (1, 2):          # n = 1: each problem alone through the single entry; n = 2: both through the group entry
        bufs = [(_padded(p['B'] * L, 256, dev), torch.full((p['B'] * 8 * L + 5,), NAN, device=dev)) for p in probs]
        args = [_attn_args(p, b[0][1], b[1], dev) for p, b in zip(probs, bufs)]
        if n == 1:
            for a in args:
                core.check(core.lib().ldetr_attention_fwd_f32(ctypes.c_void_p(a.q), a.ldq, ctypes.c_void_p(a.k), a.ldk, ctypes.c_void_p(a.v), a.ldv,
                                                              ctypes.c_void_p(a.key_padding_mask), ctypes.c_void_p(a.out), a.ldo, ctypes.c_void_p(a.lse), a.B, a.H,
                                                              a.Lq, a.Lk, a.head_dim, a.scale, a.p_drop, a.seed, ctypes.c_void_p(a.seed_ptr), 0, core.stream()), 'attention_fwd')
        else:
            arr = (_lib.AttnArgs * 2)(*args)
            assert core.lib().ldetr_attention_fwd_group_f32(arr, 2, core.stream()) == 0, 'the two problems must go out as one launch'
        torch.cuda.synchronize()
        outs.append(bufs)
    for (o1, l1), (o2, l2), p in zip(outs[0], outs[1], probs):
        assert not torch.isnan(o1[1]).any() and not torch.isnan(l1[:p['B'] * 8 * L]).any()
        assert torch.equal(bits(o1[0]), bits(o2[0])) and torch.equal(bits(l1), bits(l2))


def _max_rel(a, b):
    """Largest |a - b| / max|b| over a dict of tensors."""
    worst = 0.0
    for k in b:
        d = (a[k].double() - b[k].double()).abs().max().item()
        worst = max(worst, d / max(b[k].double().abs().max().item(), 1e-30))
    return worst


def test_encoder_pair_rider_on_equals_rider_off(dev):
    """Two 2-layer encoders (d 256, 8 heads, feed-forward 2048, dropout 0.1, train mode) with different weights: the trained one on 2 samples of 64
    tokens (128 rows), the rider on 1 (64 rows).  Off: one after the other; on: lock-step, the rider's seeds leased from its old place.
    Both memories and the trained stack's input gradient: bit-equal.  Its parameter gradients, one by one: bit-equal wherever three runs with the
    rider off are bit-equal among themselves; a parameter whose gradient is not bit-stable run to run (the backward adds it with fp32 atomics: the
    LayerNorm gains and biases; the names are printed) has no bits to compare and must stay within 3x its own off-against-off difference.  The
    backward issues the same launches (the record of its engine and token-block calls with their shapes is equal)."""
    from layoutdetr_amd.hip import blocks, core, rider
    from layoutdetr_amd.training.detr_transformer import TransformerEncoder, TransformerEncoderLayer
    torch.manual_seed(3)
    enc_a = TransformerEncoder(TransformerEncoderLayer(256, 8, 2048, 0.1), 2).to(dev).train()
    enc_b = TransformerEncoder(TransformerEncoderLayer(256, 8, 2048, 0.1), 2).to(dev).train()
    for p in enc_b.parameters():
        p.requires_grad_(False)
    xa, xb = torch.randn(128, 256, device=dev), torch.randn(64, 256, device=dev)
    pa, pb = torch.randn(128, 256, device=dev), torch.randn(64, 256, device=dev)
    ka, kb = torch.zeros(2, 64, dtype=torch.bool, device=dev), torch.zeros(1, 64, dtype=torch.bool, device=dev)
    ka[1, 60:] = True
    core.iter_seed(dev).fill_(2468)
    start = core.seed_position()
    dy = torch.randn(128, 256, device=dev)

    def run(on):
        core._seed_counter[0] = start
        for p in enc_a.parameters():
            p.grad = None
        x = xa.clone().requires_grad_(True)
        if on:
            lease = core.SeedLease(start + 8)      # the trained stack draws 2 layers x (attention, norm1, hidden, norm2) first
            (ma, mpa), (mb, mpb) = enc_a(x, 2, 64, ka, pa, want_pos=True, rider=(enc_b, xb, 1, 64, kb, pb), rider_lease=lease)
            assert lease.drawn == 8 and lease.redeem()
        else:
            ma, mpa = enc_a.forward2d(x, 2, 64, ka, pa, want_pos=True)
            with torch.no_grad():
                mb, mpb = enc_b.forward2d(xb, 1, 64, kb, pb, want_pos=True)
        assert core.seed_position() == start + 16
        launches = []      # the backward's launch record: every engine / token-block call the autograd nodes make, in order, with its shape
        real = (core.gemm, core.gemm_pair, blocks.launch)
        core.gemm = lambda A, B, ta, tb, M, N, K, **kw: (launches.append(('gemm', ta, tb, M, N, K)), real[0](A, B, ta, tb, M, N, K, **kw))[1]
        core.gemm_pair = lambda g0, g1: (launches.append(('gemm_pair',) + tuple((g['ta'], g['tb'], g['M'], g['N'], g['K']) for g in (g0, g1))), real[1](g0, g1))[1]
        blocks.launch = lambda what, args, *a, **kw: (launches.append((what, len(args))), real[2](what, args, *a, **kw))[1]
        try:
            (ma * dy).sum().backward()
        finally:
            core.gemm, core.gemm_pair, blocks.launch = real
        torch.cuda.synchronize()
        return dict(ma=ma.detach(), mpa=mpa.detach(), mb=mb, mpb=mpb, dx=x.grad.clone()), {n: p.grad.clone() for n, p in enc_a.named_parameters()}, launches
    before = dict(rider.STATS)
    offs = [run(False) for _ in range(3)]
    assert rider.STATS == before
    on, g_on, n_on = run(True)
    assert rider.STATS['paired'] - before['paired'] >= 2 * 6, rider.STATS      # per layer at least: q|k, v, attention, out-projection and the two LayerNorms
    off1, g_off1, n_off = offs[0]
    assert n_on == n_off and len(n_off) >= 2 * 4, (n_on, n_off)
    for k in off1:
        assert torch.equal(bits(off1[k]), bits(on[k])), k
    unstable = {}
    for name, g in g_off1.items():
        others = [o[1][name] for o in offs[1:]]
        if all(torch.equal(bits(g), bits(o)) for o in others):
            assert torch.equal(bits(g), bits(g_on[name])), name
        else:
            yard = max(_max_rel({name: o}, {name: g}) for o in others)
            unstable[name] = (yard, _max_rel({name: g_on[name]}, {name: g}))
    print('encoder pair, parameter gradients not bit-stable with the rider off (off against off | on against off): '
          + ', '.join(f'{n} {y:.2e} | {d:.2e}' for n, (y, d) in sorted(unstable.items())))
    assert len(unstable) < len(g_off1)
    for name, (yard, diff) in unstable.items():
        assert diff <= 3 * yard, (name, yard, diff)


def test_training_iteration_rider_on_equals_rider_off(dev):
    """Gmain + Dmain at B = 2, 64x64 backgrounds, modules in train mode (dropout on), lr 0 so that every run starts from the same weights.  Two
    iterations per run: the first measures the place of D's encoder in each phase's seed sequence, the second rides; the second is compared."""
    from layoutdetr_amd.hip import core, rider
    from layoutdetr_amd.training import training_loop as tl
    from layoutdetr_amd.training.loss import StyleGAN2Loss
    from layoutdetr_amd.training.networks_detr import Discriminator, Generator, TextFeatures
    torch.manual_seed(0)
    bg, B = 64, 2
    kw = dict(num_bbox_labels=8, img_channels=3, img_height=bg, img_width=bg, c_dim=0, background_size=bg, bert_f_dim=768, im_f_dim=512)
    G = Generator(z_dim=4, **kw).train().requires_grad_(False).to(dev)
    D = Discriminator(**kw).train().requires_grad_(False).to(dev)
    g = torch.Generator().manual_seed(1)
    batch = dict(bbox_real=torch.cat([torch.rand(B, 9, 2, generator=g) * 0.6 + 0.2, torch.rand(B, 9, 2, generator=g) * 0.35 + 0.05], -1).to(dev),
                 bbox_class=torch.randint(0, 8, (B, 9), generator=g).to(dev),
                 bbox_text=TextFeatures(torch.randn(B, 9, 768, generator=g).to(dev), torch.randint(1, 40, (B, 9), generator=g).to(dev)),
                 bbox_patch=torch.zeros(B, 9, 1, 1, 1, device=dev), padding_mask=torch.zeros(B, 9, dtype=torch.bool, device=dev),
                 background=torch.randn(B, 3, bg, bg, generator=g).to(dev), real_c=torch.zeros(B, 0, device=dev), gen_c=torch.zeros(B, 0, device=dev))
    batch['padding_mask'][1, 5:] = True
    z = [torch.randn(B, 9, 4, generator=g).to(dev) for _ in range(2)]
    start = core.seed_position()
    was = rider.ENABLED

    def run(on):
        rider.ENABLED = on
        torch.manual_seed(11)
        core._seed_counter[0] = start
        pG, pD = tl.Phase('Gmain', G, lr=0.0), tl.Phase('Dmain', D, lr=0.0)
        ema = tl.EmaTracker(pG, copy.deepcopy(G).eval())
        reports, grads, terms = {}, {}, {}
        loss = StyleGAN2Loss(dev, G, D, report_fn=lambda n, v: reports.setdefault(n, []).append(v.detach().clone()), share_D_trunk='iteration')
        dp = tl.DataParallelStep(world_size=1)
        orig = dp.apply

        def spy(phase, **k):
            for n, p in phase.module.named_parameters():
                grads[phase.name + '/' + n] = p.grad.detach().clone()
            terms.update({phase.name + '/' + k_: vs[0] for k_, vs in reports.items()})
            reports.clear()
            orig(phase, **k)
        dp.apply = spy
        for _ in range(2):
            grads.clear(); terms.clear()
            tl.training_iteration(loss, [pG, pD], dp, batch, B, z, ema=ema, batch_size=B, ema_kimg=B * 10 / 32, cur_nimg=0)
        torch.cuda.synchronize()
        return dict(terms, bbox_fake=loss.last['bbox_fake'].clone()), dict(grads)
    try:
        before = rider.STATS['paired']
        off1, g_off1 = run(False)
        off2, g_off2 = run(False)
        assert rider.STATS['paired'] == before
        on, g_on = run(True)
        assert rider.STATS['paired'] > before, 'the second iteration must ride in both phases'
    finally:
        rider.ENABLED = was
    assert set(on) == set(off1) and len(on) > 10
    for k in off1:
        assert torch.equal(bits(off1[k]), bits(on[k])), k
    yard, diff = _max_rel(g_off2, g_off1), _max_rel(g_on, g_off1)
    print(f'G+D iteration, parameter gradients: off against off {yard:.3e}, on against off {diff:.3e}')
    assert diff <= 3 * yard or diff == 0.0
