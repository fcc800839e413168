"""Training the layout-FID detector on the GPU: both paths of LayoutNet.forward (the fused launch of csrc/layoutnet_train.hip and the composed,
differentiable one) against the reference's values (tests/golden/layoutnet_train.npz) and against each other, the fused launch's
reproducibility and batch independence, gradients against a float64 restatement, the trainer's trajectory against the reference module under
torch.optim.Adam, and train_layoutnet end to end into the metric."""
import os

import numpy as np
import pytest
import torch

import layout_eval_common as C
import layoutnet_train_common as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'layoutnet_train.npz'), allow_pickle=False)
FEATURE_TOL = 2e-5      # max |delta| / max |golden|: the bar tests/test_layout_eval_gpu.py holds this transformer to
GRAD_TOL = 2e-4         # per tensor, of its largest entry: the bar tests/test_model_gpu.py holds these layers' parameter gradients to


def _net(dev, num_label):
    from layoutdetr_amd.training.networks_layoutnet import LayoutNet
    net = LayoutNet(num_label)
    net.load_state_dict(C.seeded_layoutnet_state(net), strict=True)
    return net.to(dev).eval().requires_grad_(False)


def _rel(got, want):
    want = torch.as_tensor(want).double()
    return ((got.detach().cpu().double() - want).abs().max() / want.abs().max()).item()


def _run(net, which, bbox, label, pad, dense=False):
    """forward (or forward_dense with the features) on the path `which`; a gradient asked for on the boxes sends it down the composed one."""
    from layoutdetr_amd.training import networks_layoutnet as nl
    n0 = dict(nl.PATH_RUNS)
    keep = label.clone()
    if which == 'fused':
        with torch.no_grad():
            out = net.forward_dense(bbox, label, pad, return_features=True) if dense else net(bbox, label, pad)
    else:
        with torch.enable_grad():
            b = bbox.clone().requires_grad_(True)
            out = net.forward_dense(b, label, pad, return_features=True) if dense else net(b, label, pad)
        out = tuple(o.detach() for o in out)
    other = 'composed' if which == 'fused' else 'fused'
    assert nl.PATH_RUNS['forward_' + which] == n0['forward_' + which] + 1 and nl.PATH_RUNS['forward_' + other] == n0['forward_' + other]
    assert nl.PATH_RUNS['fused'] == n0['fused'] and nl.PATH_RUNS['composed'] == n0['composed'], 'the extract_features counters count extract_features only'
    assert torch.equal(label, keep)
    return out


def _case(dev, tag):
    bbox, label, pad, is_real = T.case_inputs(tag)
    return bbox.to(dev), label.to(dev), pad.to(dev), is_real.to(dev)


@pytest.mark.parametrize('tag,which', [('A', 'fused'), ('A', 'composed'), ('B', 'fused'), ('B', 'composed'), ('C', 'composed')])
def test_forward_matches_the_reference(dev, tag, which):
    net = _net(dev, T.CASES[tag]['num_label'])
    bbox, label, pad, _ = _case(dev, tag)
    if tag == 'C':      # more than 15 elements: composed also when no gradient is asked for
        from layoutdetr_amd.training import networks_layoutnet as nl
        n0 = dict(nl.PATH_RUNS)
        with torch.no_grad():
            out = net(bbox, label, pad)
        assert nl.PATH_RUNS['forward_composed'] == n0['forward_composed'] + 1 and nl.PATH_RUNS['forward_fused'] == n0['forward_fused']
    else:
        out = _run(net, which, bbox, label, pad)
    for key, got in zip(('disc', 'cls', 'box'), out):
        want = GOLD[f'{tag}_{key}_f64']
        assert tuple(got.shape) == want.shape, (key, got.shape, want.shape)
        e = _rel(got, want)
        print(f'case {tag} {which} {key}: max |delta| / max |golden| = {e:.3e}')
        assert e <= FEATURE_TOL, (tag, which, key, e)


@pytest.mark.parametrize('tag', ['A', 'B'])
def test_fused_equals_composed(dev, tag):
    net = _net(dev, T.CASES[tag]['num_label'])
    bbox, label, pad, _ = _case(dev, tag)
    f = _run(net, 'fused', bbox, label, pad)
    c = _run(net, 'composed', bbox, label, pad)
    for key, a, b in zip(('disc', 'cls', 'box'), f, c):
        e = _rel(a, b.cpu())
        print(f'case {tag} {key}: fused vs composed {e:.3e}')
        assert a.shape == b.shape and e <= FEATURE_TOL, (tag, key, e)


def test_fused_is_reproducible_batch_independent_and_carries_the_features(dev):
    from layoutdetr_amd.training import networks_layoutnet as nl
    net = _net(dev, 13)
    bbox, label, pad, _ = _case(dev, 'A')
    a = _run(net, 'fused', bbox, label, pad, dense=True)
    b = _run(net, 'fused', bbox, label, pad, dense=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'two fused runs differ'
    # dense outputs: padded rows are 0, valid rows are what forward gathers
    assert not a[1][pad].any() and not a[2][pad].any()
    g = _run(net, 'fused', bbox, label, pad)
    assert torch.equal(g[1], a[1][~pad]) and torch.equal(g[2], a[2][~pad]) and torch.equal(g[0], a[0])
    # a padded element's box and label do not reach any output
    b2, l2 = bbox.clone(), label.clone()
    b2[pad] = 123.0
    l2[pad] = 99
    assert all(torch.equal(x, y) for x, y in zip(a, _run(net, 'fused', b2, l2, pad, dense=True))), 'padded elements changed the outputs'
    # a sample alone = the same sample inside the batch of 18, bit for bit
    for i in (0, 8, 17):
        one = _run(net, 'fused', bbox[i:i + 1], label[i:i + 1], pad[i:i + 1], dense=True)
        assert all(torch.equal(x[i:i + 1], y) for x, y in zip(a, one)), i
    # the features output is ldetr_layoutnet_features_f32's, bit for bit (the same input stage and layer body, csrc/layoutnet_layers.hpp)
    with torch.no_grad():
        assert torch.equal(a[3], net.extract_features(bbox, label, pad))
    # 257 samples: the three-samples-per-block launch with a ragged last block against the first 257 rows in chunks of at most 256 (one sample per
    # block).  BIT FOR BIT: a sample's arithmetic is the same sequence of MFMAs, shuffles and LDS reductions whichever block shape holds it -- the
    # samples of a block share weight tiles, never accumulators.
    big = tuple(t.to(dev) for t in C.seeded_layouts('train.big', n=257, N=9, num_label=13))
    whole = _run(net, 'fused', *big, dense=True)
    parts = [_run(net, 'fused', *(t[s] for t in big), dense=True) for s in (slice(0, 256), slice(256, 257))]
    for k in range(4):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    with torch.no_grad():
        assert torch.equal(whole[3], net.extract_features(*big))
    assert all(torch.isfinite(t).all() for t in whole)


def test_bad_label_poisons_its_sample_only(dev):
    net = _net(dev, 13)
    bbox, label, pad, _ = _case(dev, 'A')
    ref = _run(net, 'fused', bbox, label, pad, dense=True)
    bad = label.clone()
    bad[5, 0] = 13                # sample 5 has six valid elements
    out = _run(net, 'fused', bbox, bad, pad, dense=True)
    others = [i for i in range(bbox.shape[0]) if i != 5]
    assert torch.isnan(out[0][5]) and torch.isnan(out[3][5]).all()
    assert torch.isnan(out[1][5][~pad[5]]).all() and torch.isnan(out[2][5][~pad[5]]).all() and not out[1][5][pad[5]].any() and not out[2][5][pad[5]].any()
    assert all(torch.equal(o[others], r[others]) for o, r in zip(out, ref))
    # the same label in a padded slot is not read
    bad = label.clone()
    bad[0, 8] = 13
    assert pad[0, 8] and all(torch.equal(o, r) for o, r in zip(_run(net, 'fused', bbox, bad, pad, dense=True), ref))


def test_gradients_match_a_float64_restatement(dev):
    """Composed path, eval mode, case A with alternating is_real: every parameter's gradient and the boxes' against autograd through
    tests/layoutnet_train_common.forward_ref in float64 on the host.  Per tensor max |delta| <= GRAD_TOL x its largest entry (the reference's
    own float32 run is 1.0e-6 from its float64 run on these gradients)."""
    from layoutdetr_amd.train_layoutnet import detector_loss
    from layoutdetr_amd.training import networks_layoutnet as nl
    bbox, label, pad, is_real = T.case_inputs('A')
    net = _net(dev, 13).requires_grad_(True)
    b = bbox.to(dev).requires_grad_(True)
    n0 = dict(nl.PATH_RUNS)
    terms, total = detector_loss(net, b, label.to(dev), pad.to(dev), is_real.to(dev))
    assert nl.PATH_RUNS['forward_composed'] == n0['forward_composed'] + 1 and nl.PATH_RUNS['forward_fused'] == n0['forward_fused']
    total.backward()
    sd = {k: (v.requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in T.to_dtype(C.seeded_layoutnet_state(nl.LayoutNet(13)), torch.float64).items()}
    b64 = bbox.double().requires_grad_(True)
    l_disc, l_cls, l_bbox, tot64 = T.loss_ref(sd, b64, label, pad, is_real)
    tot64.backward()
    for name, got, want in (('L_disc', terms['L_disc'], l_disc), ('L_cls', terms['L_cls'], l_cls), ('L_bbox', terms['L_bbox'], l_bbox), ('total', terms['total'], tot64)):
        e = abs(got.item() - want.item()) / abs(want.item())
        print(f'{name}: {got.item()!r} vs {want.item()!r} ({e:.2e})')
        assert e <= FEATURE_TOL, name
    for got, want in zip((terms['L_disc'], terms['L_cls'], terms['L_bbox']), GOLD['A_loss_terms']):
        assert abs(got.item() - want) <= FEATURE_TOL * abs(want)
    worst = ('', 0.0)
    for name, p in list(net.named_parameters()) + [('bbox', b)]:
        want = (b64 if name == 'bbox' else sd[name]).grad
        assert p.grad is not None and want is not None, name
        e = ((p.grad.detach().cpu().double() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()
        worst = max(worst, (name, e), key=lambda t: t[1])
        assert e <= GRAD_TOL, (name, e)
    print(f'worst gradient: {worst[0]} {worst[1]:.3e}')


def test_trainer_follows_the_reference_trajectory(dev):
    """LayoutNetTrainer.step (composed forward, hip/losses tail, flat fused Adam; dropout 0) on the fixture's eight batches: each step's total loss
    within 2e-5 relative of the reference module's float64 run under torch.optim.Adam (12 x what the reference's own float32 run needs, 1.6e-6); each
    term within 2e-5 of the total's size (a term enters the total with that absolute error; the small box term alone is 1.0e-5 relative in the
    reference's float32 run).  Afterwards the fused features equal the composed ones: the packed weights followed the optimiser."""
    from layoutdetr_amd.train_layoutnet import LayoutNetTrainer
    t = T.TRAJ
    net = _net(dev, t['num_label'])
    trainer = LayoutNetTrainer(net, lr=t['lr'], betas=t['betas'], eps=t['eps'], dropout=0.0, w_bbox=T.W_BBOX)
    batches = [tuple(x.to(dev) for x in b) for b in T.trajectory_batches()]
    with torch.no_grad():
        before = net.eval().extract_features(*batches[0][:3])      # packs the weights: the copy the optimiser must not leave behind
    rows = []
    for bbox, label, pad, is_real in batches:
        terms = trainer.step(bbox, label, pad, is_real)
        assert all(v.is_cuda and not v.requires_grad for v in terms.values())
        rows.append(torch.stack([terms[k] for k in ('L_disc', 'L_cls', 'L_bbox', 'total')]))
    got = torch.stack(rows).double().cpu().numpy()
    want = GOLD['traj_losses_f64']
    for k in range(t['steps']):
        e = np.abs(got[k] - want[k]) / np.abs(want[k, 3])
        print(f'step {k}: total {got[k, 3]!r} vs {want[k, 3]!r}; errors / total: {e}')
    assert (np.abs(got[:, 3] - want[:, 3]) <= 2e-5 * np.abs(want[:, 3])).all()
    assert (np.abs(got[:, :3] - want[:, :3]) <= 2e-5 * np.abs(want[:, 3:4])).all()
    assert got[-1, 3] < got[0, 3]
    net.eval()
    with torch.no_grad():
        fused = net.extract_features(*batches[0][:3])
    with torch.enable_grad():
        composed = net.extract_features(batches[0][0].clone().requires_grad_(True), *batches[0][1:3]).detach()
    e = _rel(fused, composed.cpu())
    print(f'after 8 steps: fused vs composed features {e:.3e}; moved by {_rel(fused, before.cpu()):.3e}')
    assert e <= FEATURE_TOL and not torch.equal(fused, before)
    ev = trainer.evaluate(batches[0][0], batches[0][1], ~batches[0][2], is_real=batches[0][3])
    assert all(np.isfinite(v) for v in ev.values()) and 0.0 <= ev['cls_acc'] <= 1.0 and 0.0 <= ev['disc_acc'] <= 1.0


def test_train_layoutnet_writes_the_file_the_metric_loads(dev, tmp_path, monkeypatch):
    from layoutdetr_amd.metrics import metric_main
    from layoutdetr_amd.train_layoutnet import train_layoutnet
    from layoutdetr_amd.training.networks_layoutnet import LayoutNet
    zpath = C.stage_dataset(tmp_path)
    monkeypatch.chdir(tmp_path)
    ds = dict(class_name='layoutdetr_amd.training.dataset_layoutganpp.LayoutDataset', path=zpath, use_labels=False, max_size=None, xflip=False, background_size=32)
    lines = []
    out, last = train_layoutnet(ds, steps=20, batch=8, eval_every=10, log=lines.append)
    assert out == f'pretrained/layoutnet_{C.DATASET_NAME}.pth.tar' and os.path.isfile(tmp_path / out)
    assert [f for f in os.listdir(tmp_path / 'pretrained')] == [os.path.basename(out)], 'a temporary file was left behind'
    assert sum(l.startswith('step') for l in lines) == 2 and all(np.isfinite(v) for v in last.values())
    sd = torch.load(tmp_path / out, map_location='cpu')
    want = LayoutNet(13).state_dict()
    assert sorted(sd) == sorted(want) and all(sd[k].shape == want[k].shape and sd[k].dtype == want[k].dtype for k in want)
    assert all(v.untyped_storage().nbytes() == v.numel() * v.element_size() for v in sd.values()), 'tensors must be saved as plain tensors, not views of the flat buffer'
    r = metric_main.calc_metric('layout_fid50k_train', cache=False, G=C.StubGenerator().to(dev), dataset_kwargs=ds, num_gpus=1, rank=0, device=dev)
    fid = r.results['layout_fid50k_train']
    print('layout FID with the trained detector:', fid)
    assert np.isfinite(fid)
