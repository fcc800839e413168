"""GPU tests of layout generation: the finishing kernel (csrc/layout_finish.hip) against the reference's own results (fixture
tests/golden/generate.npz) and against a plain restatement on edge shapes, the shared-condition decode (training/shared_decode.py) against the
unchanged Generator.forward and the CPU oracle, the reuse of a Condition, and generate_layouts end to end from strings."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'generate.npz')
F = np.float32


def stable_order(ov):
    """np.argsort(kind='stable') places NaN last."""
    return np.argsort(ov, kind='stable')


# ---------------------------------------------------------------------------------------------------------------------------------
# finishing kernel against the reference's results


def test_layout_finish_matches_reference_fixture(dev):
    """Every kept case of the fixture in ONE launch as C = 2 groups (the second group's indexing is exercised).  Boxes within 1e-6 absolute
    (about 6x the reference's own fp32 / fp64 spread on the kept cases), overlap / alignment within 5e-5 relative + 1e-6 (the bar of the
    layout-loss golden test), order EQUAL to the stable argsort of the overlaps the device returned."""
    from layoutdetr_amd.generate import layout_finish
    g = np.load(GOLDEN, allow_pickle=False)
    n = g['bbox_in'].shape[0]
    assert n >= 230 and float(g['fp64_box_spread']) < 1e-6 / 3
    K = (n + 1) // 2
    idx = np.minimum(np.arange(2 * K), n - 1)          # an odd count: the last case is fed twice, so that EVERY kept case reaches the kernel
    assert set(idx.tolist()) == set(range(n))
    grouped = lambda a: np.ascontiguousarray(a[idx]).reshape((2, K) + a.shape[1:])
    t = lambda a, dt: torch.from_numpy(grouped(a)).to(dev).to(dt)
    out, ov, al, order = layout_finish(t(g['bbox_in'], torch.float32), t(g['num'], torch.int32), t(g['factors'], torch.float32),
                                       t(g['jitter'], torch.uint8), t(g['mode'], torch.uint8))
    torch.cuda.synchronize()
    out, ov, al, order = out.cpu().numpy(), ov.cpu().numpy(), al.cpu().numpy(), order.cpu().numpy()
    ref = lambda k: grouped(g[k])
    eb = np.abs(out.astype(np.float64) - ref('bbox_out')).max()
    eo = (np.abs(ov.astype(np.float64) - ref('overlap')) - 5e-5 * np.abs(ref('overlap'))).max()
    ea = (np.abs(al.astype(np.float64) - ref('alignment')) - 5e-5 * np.abs(ref('alignment'))).max()
    print(f'layout_finish vs reference: boxes {eb:.3e}, overlap excess {eo:.3e}, alignment excess {ea:.3e} ({n} cases)')
    assert eb <= 1e-6, f'boxes differ by {eb:.3e}'
    assert eo <= 1e-6, f'overlap beyond 5e-5 relative + 1e-6 by {eo - 1e-6:.3e}'
    assert ea <= 1e-6, f'alignment beyond 5e-5 relative + 1e-6 by {ea - 1e-6:.3e}'
    for c in range(2):
        assert np.array_equal(order[c], stable_order(ov[c])), f'group {c}: order is not the stable argsort of the returned overlaps'
    assert (ov == 0).sum() >= 2, 'the fixture must hold ties at exactly 0 (stability is part of the contract)'


# ---------------------------------------------------------------------------------------------------------------------------------
# finishing kernel on edge shapes against a plain restatement


def restate(box, num, fac, jit, mode):
    """generate_util.py:100-148 + metrics/metric_layoutnet.py:153-201 on ONE layout, float32 scalars in the reference's operation order.
    -> (boxes [N, 4], overlap, alignment, smallest margin of a de_overlap decision)."""
    b = box.astype(F).copy()
    N = b.shape[0]
    h = F(2)
    margin = np.inf
    if jit and fac is not None:
        b = (b * fac.astype(F)).astype(F)
    if mode == 1:
        s = F(0)
        for i in range(num):
            s = F(s + b[i, 0])
        b[:, 0] = F(s / F(num))
    elif mode == 2:
        s = F(0)
        for i in range(num):
            s = F(s + F(b[i, 0] - F(b[i, 2] / h)))
        m = F(s / F(num))
        for i in range(num):
            x1 = F(b[i, 0] - F(b[i, 2] / h))
            b[i, 0] = F(b[i, 0] - F(x1 - m))
    if mode in (1, 2):
        for pas in (0, 1):
            for i in range(num):
                for j in range(num):
                    if i == j:
                        continue
                    hh = F(F(b[i, 3] / h) + F(b[j, 3] / h))
                    ad = F(abs(F(b[j, 1] - b[i, 1])))
                    margin = min(margin, abs(float(ad) - float(hh)))
                    if ad < hh:
                        half = F(F(hh - ad) / h)
                        if pas == 0:
                            margin = min(margin, abs(float(b[i, 1]) - float(b[j, 1])))
                            if b[i, 1] < b[j, 1]:
                                b[i, 1] = F(b[i, 1] - half); b[j, 1] = F(b[j, 1] + half)
                            else:
                                b[i, 1] = F(b[i, 1] + half); b[j, 1] = F(b[j, 1] - half)
                        else:
                            b[i, 3] = F(b[i, 3] - half); b[j, 3] = F(b[j, 3] - half)
    ltrb = lambda x: (F(x[0] - F(x[2] / h)), F(x[1] - F(x[3] / h)), F(x[0] + F(x[2] / h)), F(x[1] + F(x[3] / h)))
    ov = F(0)
    for i in range(num):
        l1, t1, r1, b1 = ltrb(b[i])
        a1 = F(F(r1 - l1) * F(b1 - t1))
        for j in range(num):
            if j == i:
                continue
            l2, t2, r2, b2 = ltrb(b[j])
            lm, rm, tm, bm = max(l1, l2), min(r1, r2), max(t1, t2), min(b1, b2)
            if lm < rm and tm < bm:
                with np.errstate(all='ignore'):
                    ov = F(ov + np.nan_to_num(F(F(F(rm - lm) * F(bm - tm)) / a1)))
    with np.errstate(all='ignore'):
        ov = F(ov / F(num))
    X = np.stack([b[:, 0] - b[:, 2] / h, b[:, 0], b[:, 0] + b[:, 2] / h, b[:, 1] - b[:, 3] / h, b[:, 1], b[:, 1] + b[:, 3] / h]).astype(F)      # [6, N]
    D = np.abs(X[:, :, None] - X[:, None, :]).astype(F)
    D[:, np.arange(N), np.arange(N)] = F(1)
    al = F(0)
    for i in range(num):
        best = D[:, i, :].min()               # a minimum does not depend on the order it is taken in
        if best != F(1):
            al = F(al + F(-np.log(F(F(1) - best))))
    with np.errstate(all='ignore'):
        al = F(al / F(num))
    return b, ov, al, margin


VARIANTS = ['num1', 'num9', 'mode0_jitter_all', 'mode0_jitter_none', 'mode0_jitter_mixed', 'no_factors', 'mixed', 'n16', 'n5']


@pytest.mark.parametrize('K', [1, 17, 65])          # less than, off, and just past a wave
@pytest.mark.parametrize('variant', VARIANTS)
def test_layout_finish_edge_shapes_vs_restatement(dev, K, variant):
    _check_against_restatement(dev, K, variant)


def test_layout_finish_more_candidates_than_threads(dev):
    """K = 300 > the block's 128 threads: a thread finishes candidates k, k + 128, k + 256 in turn, reusing its LDS column, and ranks over all 300."""
    _check_against_restatement(dev, 300, 'mixed')


def _check_against_restatement(dev, K, variant):
    from layoutdetr_amd.generate import layout_finish
    C = 2
    N = {'n16': 16, 'n5': 5}.get(variant, 9)
    rs = np.random.RandomState(1000 + K + 7 * VARIANTS.index(variant))
    box = (1 / (1 + np.exp(-rs.randn(C, K, N, 4)))).astype(F)
    fac = np.exp(rs.uniform(np.log(0.8), np.log(1.2), (C, K, N, 4))).astype(F)
    num = rs.randint(1, N + 1, (C, K)).astype(np.int32)
    mode = rs.randint(0, 3, (C, K)).astype(np.uint8)
    jit = rs.randint(0, 2, (C, K)).astype(np.uint8)
    if variant == 'num1':
        num[:] = 1
    elif variant == 'num9':
        num[:] = 9
    elif variant.startswith('mode0'):
        mode[:] = 0
        jit[:] = {'all': 1, 'none': 0}.get(variant.split('_')[-1], jit)
    use_fac = variant != 'no_factors'
    d = lambda a: torch.from_numpy(a).to(dev)
    out, ov, al, order = layout_finish(d(box), d(num), d(fac) if use_fac else None, d(jit), d(mode))
    torch.cuda.synchronize()
    out, ov, al, order = out.cpu().numpy(), ov.cpu().numpy(), al.cpu().numpy(), order.cpu().numpy()
    assert order.dtype == np.int32 and out.shape == box.shape
    checked = 0
    for c in range(C):
        assert np.array_equal(order[c], stable_order(ov[c])), f'group {c}: order is not the stable argsort of the returned overlaps'
        for k in range(K):
            rb, ro, ra, margin = restate(box[c, k], int(num[c, k]), fac[c, k] if use_fac else None, bool(jit[c, k]), int(mode[c, k]))
            if margin < 1e-4:                     # a de_overlap decision closer than 1e-4 to its threshold pins nothing
                continue
            checked += 1
            assert np.abs(out[c, k].astype(np.float64) - rb).max() <= 1e-6, (c, k)
            assert abs(float(ov[c, k]) - float(ro)) <= 5e-5 * abs(float(ro)) + 1e-6, (c, k, ov[c, k], ro)
            assert abs(float(al[c, k]) - float(ra)) <= 5e-5 * abs(float(ra)) + 1e-6, (c, k, al[c, k], ra)
    assert checked >= max(1, (C * K) // 2), f'only {checked} of {C * K} layouts had decision margins >= 1e-4'
    if variant == 'num1':                         # no pairs: every overlap is exactly 0 and the order is the identity
        assert (ov == 0).all() and np.array_equal(order, np.tile(np.arange(K, dtype=np.int32), (C, 1)))
    if variant == 'mode0_jitter_none':
        assert np.array_equal(out, box)
    if variant == 'mode0_jitter_all':
        assert np.array_equal(out, (box * fac).astype(F))


def test_layout_finish_ranks_nan_last_and_ties_by_index(dev):
    """num = 0 gives 0 / 0 = NaN overlaps (as the reference's division by an empty mask does); they rank after every number, in index order."""
    from layoutdetr_amd.generate import layout_finish
    K = 6
    box = torch.tensor([[0.5, 0.5, 0.4, 0.4]] * 9, device=dev).repeat(1, K, 1, 1)      # nine identical boxes: overlap > 0 wherever num >= 2
    num = torch.tensor([[0, 2, 1, 0, 3, 1]], dtype=torch.int32, device=dev)
    _, ov, _, order = layout_finish(box, num)
    ov, order = ov.cpu().numpy()[0], order.cpu().numpy()[0]
    assert np.isnan(ov[[0, 3]]).all() and (ov[[2, 5]] == 0).all() and ov[1] > 0 and ov[4] > 0
    assert order.tolist() == stable_order(ov).tolist() and order.tolist()[:2] == [2, 5] and order.tolist()[-2:] == [0, 3]


# ---------------------------------------------------------------------------------------------------------------------------------
# shared-condition decode


def _make_G(dev, bg, seed=0, **kw):
    """A small Generator as tests/test_model_gpu.py::_make builds one: z_dim 4, non-trivial FrozenBN statistics."""
    from layoutdetr_amd.training.networks_detr import Generator
    torch.manual_seed(seed)
    G = Generator(z_dim=4, num_bbox_labels=8, img_channels=3, img_height=bg, img_width=bg, c_dim=0, background_size=bg, bert_f_dim=768, im_f_dim=512, **kw)
    for m in G.modules():
        if m.__class__.__name__ == 'FrozenBatchNorm2d':
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1); m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
    return G


def _condition_inputs(bg, seed=1):
    g = torch.Generator().manual_seed(seed)
    C = 2
    d = dict(bbox_class=torch.randint(0, 8, (C, 9), generator=g), text_feat=torch.randn(C, 9, 768, generator=g), text_len=torch.randint(1, 40, (C, 9), generator=g),
             background=torch.randn(C, 3, bg, bg, generator=g), padding_mask=torch.arange(9)[None, :] >= torch.tensor([[6], [9]]))      # padded lengths 6 and 9
    return d, torch.randn(3, 9, 4, generator=g)      # K = 3 candidates


@pytest.mark.parametrize('bg', [64, 288])            # 4 and 81 memory tokens: below and above the 64-key limit of the short-sequence kernels
def test_shared_decode_equals_forward_and_oracle(dev, bg):
    from layoutdetr_amd.generate import Sampler
    from layoutdetr_amd.training.networks_detr import TextFeatures
    from oracle import detr_ref, networks_ref
    G = _make_G(dev, bg)
    d, z = _condition_inputs(bg)
    C, K = 2, z.shape[0]
    sd = {k: v.clone() for k, v in G.state_dict().items()}
    with torch.no_grad():
        feats = detr_ref.resnet50_layer4(sd, 'backbone.0.body.', d['background'])        # the oracle's trunk once per background, shared by its K calls
        rep = lambda t: t.repeat_interleave(K, 0)
        ref = networks_ref.generator(sd, z.repeat(C, 1, 1), rep(d['bbox_class']), rep(d['text_feat']), rep(d['text_len']), rep(d['padding_mask']),
                                     rep(d['background']), feats=rep(feats)).reshape(C, K, 9, 4)
    G.eval().requires_grad_(False).to(dev)
    s = Sampler(G)
    t = {k: v.to(dev) for k, v in d.items()}
    cond = s.encode(t['background'], TextFeatures(t['text_feat'], t['text_len']), t['bbox_class'], padding_mask=t['padding_mask'])
    assert cond.S == ((bg + 31) // 32) ** 2 and cond.num.tolist() == [6, 9]
    res = s.sample(cond, z=z.to(dev))
    patch = torch.zeros(1, 9, 1, 1, 1, device=dev)
    worst_fwd = worst_ref = 0.0
    with torch.no_grad():
        for c in range(C):
            tf = TextFeatures(t['text_feat'][c:c + 1], t['text_len'][c:c + 1])
            valid = ~d['padding_mask'][c]
            for k in range(K):
                one = G(z[k:k + 1].to(dev), t['bbox_class'][c:c + 1], None, tf, patch, t['padding_mask'][c:c + 1], t['background'][c:c + 1], None)[0]
                worst_fwd = max(worst_fwd, (res.bbox_raw[c, k] - one).abs().max().item())
                worst_ref = max(worst_ref, ((res.bbox_raw[c, k].cpu() - ref[c, k])[valid].abs().max() / ref[c, k][valid].abs().max()).item())
    print(f'shared decode, background {bg}: vs forward {worst_fwd:.3e} absolute, vs oracle {worst_ref:.3e} relative')
    assert worst_fwd <= 2e-5, f'bbox_raw differs from Generator.forward by {worst_fwd:.3e}'
    assert worst_ref <= 1e-3, f'bbox_raw differs from the oracle by {worst_ref:.3e} relative'
    assert torch.equal(res.bbox, res.bbox_raw) and res.modes == [0, 0, 0]                # no plan: nothing is finished


@pytest.mark.parametrize('n_each', [3, 70])          # 3 + 3 stay inside one decoder pass; 70 + 70 = 140 candidates cross into a second one
def test_condition_is_reusable_without_the_trunk(dev, n_each):
    """Two sample calls with different seeds on one Condition == one call with the concatenated seeds, bit for bit; the second call launches no
    trunk kernel (the engine launch counters of the C ABI: its contraction launches equal the first call's and do not depend on the background)."""
    from layoutdetr_amd.generate import CENTER, LEFT, Sampler
    from layoutdetr_amd.hip import core
    from layoutdetr_amd.training import shared_decode
    from layoutdetr_amd.training.networks_detr import TextFeatures
    assert n_each <= shared_decode.CHUNK < 2 * 70, 'the cases are chosen around the candidates of one decoder pass'
    sa, sb = list(range(3, 3 + n_each)), [9, 1, 2] + list(range(40, 40 + n_each - 3))
    plan = lambda seeds: dict(jitter=[s % 3 != 1 for s in seeds], modes=[CENTER if s % 2 else LEFT for s in seeds])
    per_call = {}
    for bg in (64, 128):
        G = _make_G(dev, bg).eval().requires_grad_(False).to(dev)
        d, _ = _condition_inputs(bg)
        t = {k: v.to(dev) for k, v in d.items()}
        s = Sampler(G)
        n0 = sum(core.engine_launch_counts())
        cond = s.encode(t['background'], TextFeatures(t['text_feat'], t['text_len']), t['bbox_class'], padding_mask=t['padding_mask'])
        n1 = sum(core.engine_launch_counts())
        a = s.sample(cond, seeds=sa, **plan(sa))
        n2 = sum(core.engine_launch_counts())

        def no_trunk(*args, **kw):
            raise AssertionError('the trunk ran during sample()')
        G.trunk = no_trunk
        G.backbone.forward = no_trunk
        b = s.sample(cond, seeds=sb, **plan(sb))
        n3 = sum(core.engine_launch_counts())
        both = s.sample(cond, seeds=sa + sb, **plan(sa + sb))
        assert tuple(both.bbox_raw.shape) == (2, 2 * n_each, 9, 4)
        for name in ('bbox_raw', 'bbox', 'overlap', 'alignment'):
            assert torch.equal(torch.cat([getattr(a, name), getattr(b, name)], dim=1), getattr(both, name)), name
        assert not torch.equal(a.bbox_raw, b.bbox_raw)
        assert n1 - n0 > 0 and n2 - n1 > 0 and n3 - n2 == n2 - n1, (n0, n1, n2, n3)
        per_call[bg] = n3 - n2
    assert per_call[64] == per_call[128], f'sample() launches depend on the background size: {per_call}'


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end from strings


def test_generate_layouts_end_to_end_from_strings(dev, tmp_path):
    from layoutdetr_amd.generate import CENTER, LEFT, NONE, generate_layouts, layout_finish, jitter_factors
    vocab = ['[PAD]', '[unused0]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', 'sale', 'up', 'to', '50', '%', 'off', 'shop', 'now', 'free', 'ship', '##ping', 'on', 'order', '##s']
    vf = tmp_path / 'vocab.txt'
    vf.write_text('\n'.join(vocab) + '\n', encoding='utf-8')
    bg = 64
    G = _make_G(dev, bg, seed=3, text_mode='encoder', tokenizer_vocab=str(vf), bert_num_encoder_layers=2, bert_num_heads=4).to(dev)
    pages = torch.randint(0, 256, (2, 40, 56, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)      # uint8 pages of another size
    texts = [['Sale', 'Up to 50% off', 'Shop now'], ['Free shipping on orders']]
    labels = [[0, 3, 5], [3]]
    seeds = [1, 2, 3, 4, 5]
    plan = [(False, CENTER), (True, LEFT), (True, CENTER), (False, NONE), (True, NONE)]
    res = generate_layouts(G, pages, texts, labels, seeds, post_process=plan, background_size=bg)
    C, K = 2, len(seeds)
    assert tuple(res.bbox_raw.shape) == tuple(res.bbox.shape) == (C, K, 9, 4)
    assert tuple(res.overlap.shape) == tuple(res.alignment.shape) == tuple(res.order.shape) == (C, K)
    assert res.num.tolist() == [3, 1] and res.seeds == seeds
    assert torch.isfinite(res.bbox_raw).all() and (res.bbox_raw > 0).all() and (res.bbox_raw < 1).all()
    for c in range(C):
        assert sorted(res.order[c].tolist()) == list(range(K))
        assert res.order[c].tolist() == stable_order(res.overlap[c].cpu().numpy()).tolist()
    assert (res.overlap[1] == 0).all() and res.order[1].tolist() == list(range(K))       # one element: nothing overlaps, ties keep their order
    # bbox is the finishing launch applied to bbox_raw
    flags = torch.tensor([[p[0] for p in plan]], dtype=torch.uint8, device=dev)
    modes = torch.tensor([[p[1] for p in plan]], dtype=torch.uint8, device=dev)
    again = layout_finish(res.bbox_raw, res.num, jitter_factors(seeds).to(dev).unsqueeze(0), flags, modes)
    assert torch.equal(again[0], res.bbox) and torch.equal(again[1], res.overlap) and torch.equal(again[3], res.order)
    assert torch.equal(res.bbox[:, 3], res.bbox_raw[:, 3]) and not torch.equal(res.bbox[:, 4], res.bbox_raw[:, 4])
    assert (res.bbox[0, 0, :, 0] == res.bbox[0, 0, 0, 0]).all()                         # centre mode: one xc for all slots

    # the command line on a snapshot of this G (training_loop.save_snapshot's format: a pickle of dict(G=, D=, G_ema=) modules)
    import copy
    import json
    import pickle
    import PIL.Image
    from layoutdetr_amd import generate
    with open(tmp_path / 'snap.pkl', 'wb') as f:
        pickle.dump(dict(G=None, D=None, G_ema=copy.deepcopy(G).cpu(), augment_pipe=None, training_set_kwargs={}), f)
    PIL.Image.fromarray(pages[0].cpu().numpy()).save(tmp_path / 'bg.png')
    generate.main(['--ckpt', str(tmp_path / 'snap.pkl'), '--bg', str(tmp_path / 'bg.png'), '--bg-preprocessing', '128', '--strings', 'Sale|Shop now',
                   '--string-labels', 'header|button', '--seeds', '1,3-4', '--out-postprocessing', 'horizontal_left_aligned', '--out-jittering-strength', '0.1',
                   '--outfile', str(tmp_path / 'out' / 'x')])
    out = json.load(open(tmp_path / 'out' / 'x.json'))
    assert out['seeds'] == [1, 3, 4] and sorted(out['order']) == [0, 1, 2] and np.array(out['bbox']).shape == (3, 2, 4) and len(out['overlap']) == 3
    assert out['labels'] == ['header', 'button'] and all(p['mode'] == 'horizontal_left_aligned' and p['jitter'] for p in out['plan'])
    assert PIL.Image.open(tmp_path / 'out' / 'x_bboxes.png').size == (56, 40)
