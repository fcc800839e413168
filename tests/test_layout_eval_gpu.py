"""Layout metrics on the GPU: the fused LayoutNet feature kernel and the float64 statistics kernel (csrc/layoutnet.hip) against the reference's
values (tests/golden/layout_eval.npz, tools/gen_layout_eval_golden.py) and against the composed path; the metric passes, the registry's
calc_metric / report_metric, training_loop(metrics=...) and the two-rank combination."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import layout_eval_common as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'layout_eval.npz'), allow_pickle=False)
FEATURE_TOL = 2e-5      # max |delta| / max |golden|: the bar tests/test_model_gpu.py holds the same transformer to
MEANS = ('overlap_50k_train', 'alignment_50k_train', 'layoutwise_iou50k_train', 'layoutwise_docsim50k_train')
FID_NAME, MEANS_NAME = 'layout_fid50k_train', 'overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k_train'


def _net(dev, num_label=C.NUM_LABEL):
    from layoutdetr_amd.training.networks_layoutnet import LayoutNet
    net = LayoutNet(num_label)
    net.load_state_dict(C.seeded_layoutnet_state(net), strict=True)
    return net.to(dev).eval().requires_grad_(False)


def _to(dev, triple):
    return tuple(t.to(dev) for t in triple)


def _rel(got, want):
    want = torch.as_tensor(want).double()
    return ((got.detach().cpu().double() - want).abs().max() / want.abs().max()).item()


def _composed(net, bbox, label, pad, **kw):
    """extract_features through the composed path: with a gradient asked for on the boxes the fused kernel does not apply."""
    from layoutdetr_amd.training import networks_layoutnet as nl
    n0 = dict(nl.PATH_RUNS)
    with torch.enable_grad():
        out = net.extract_features(bbox.clone().requires_grad_(True), label, pad, **kw).detach()
    assert nl.PATH_RUNS['composed'] == n0['composed'] + 1 and nl.PATH_RUNS['fused'] == n0['fused']
    return out


def _fused(net, bbox, label, pad, **kw):
    from layoutdetr_amd.training import networks_layoutnet as nl
    n0 = dict(nl.PATH_RUNS)
    with torch.no_grad():
        out = net.extract_features(bbox, label, pad, **kw)
    assert nl.PATH_RUNS['fused'] == n0['fused'] + 1 and nl.PATH_RUNS['composed'] == n0['composed']
    return out


def test_extract_features_match_the_reference_on_both_paths(dev):
    net = _net(dev)
    bbox, label, pad = _to(dev, C.seeded_layouts('real'))
    cases = [('features_real256', (bbox[:256], label[:256], pad[:256]), {}),
             ('features_replace', (bbox[:64], label[:64] % 8, pad[:64]), dict(label_idx_replace=True)),
             ('features_replace2', (bbox[:64], label[:64] % 5, pad[:64]), dict(label_idx_replace_2=True))]
    for key, args, kw in cases:
        keep = args[1].clone()
        for name, fn in (('fused', _fused), ('composed', _composed)):
            got = fn(net, *args, **kw)
            assert got.shape == GOLD[key].shape
            e = _rel(got, GOLD[key])
            print(f'{key} {name}: max |delta| / max |golden| = {e:.3e}')
            assert e <= FEATURE_TOL, (key, name, e)
        assert torch.equal(args[1], keep), 'the caller\'s labels were modified'
    # more than 15 elements: a sample no longer fits the 16-row tile -> the composed path, also without a gradient
    from layoutdetr_amd.training import networks_layoutnet as nl
    b20, l20, p20 = _to(dev, C.seeded_layouts('long', n=4, N=20))
    n0 = dict(nl.PATH_RUNS)
    with torch.no_grad():
        out = net.extract_features(b20, l20, p20)
    assert nl.PATH_RUNS['composed'] == n0['composed'] + 1 and nl.PATH_RUNS['fused'] == n0['fused']
    assert out.shape == (4, 256) and torch.isfinite(out).all()


def test_fused_features_equal_the_composed_path_and_are_reproducible(dev):
    net = _net(dev)
    worst = 0.0
    for tag in ('real', 'fake'):
        bbox, label, pad = _to(dev, C.seeded_layouts(tag))
        f = _fused(net, bbox, label, pad)
        c = torch.cat([_composed(net, bbox[i:i + 256], label[i:i + 256], pad[i:i + 256]) for i in range(0, bbox.shape[0], 256)])
        e = _rel(f, c.cpu())
        print(f'{tag}: fused vs composed, 1024 layouts: {e:.3e}')
        worst = max(worst, e)
        assert e <= FEATURE_TOL
        assert torch.equal(f, _fused(net, bbox, label, pad)), 'two fused runs differ'
        # the small-batch launch (one sample per block) and the large-batch launch (three per block) are the same arithmetic
        assert torch.equal(f[:8], _fused(net, bbox[:8], label[:8], pad[:8]))
        # a padded element's box and label do not reach the output
        b2, l2 = bbox.clone(), label.clone()
        b2[pad] = 123.0
        l2[pad] = 99
        assert torch.equal(f, _fused(net, b2, l2, pad)), 'padded elements changed the features'
    # a VALID element with a label outside the embedding table: that sample's features are NaN, the others are untouched
    bbox, label, pad = _to(dev, C.seeded_layouts('real', n=4))
    ref = _fused(net, bbox, label, pad)
    bad = label.clone(); bad[2, 0] = 13
    out = _fused(net, bbox, bad, pad)
    assert torch.isnan(out[2]).all() and torch.equal(out[[0, 1, 3]], ref[[0, 1, 3]])


def _bound(x64):
    return 1e-12 * (np.abs(x64).T @ np.abs(x64)), 1e-12 * np.abs(x64).sum(0)


def test_feature_stats_f64_kernel(dev):
    """raw_mean / raw_cov against numpy float64: elementwise |delta| <= 1e-12 (|x|^T |x|) (the worst-case summation bound n 2^-53 = 1.1e-13 at
    n = 1024, times 10)."""
    from layoutdetr_amd.metrics.metric_utils_layout import FeatureStats
    from oracle import seeded
    x = (seeded.uniform('layout_eval.stats.x', (1024, 256), 9, -2.0, 3.0) * seeded.uniform('layout_eval.stats.s', (1, 256), 9, 0.01, 10.0)).to(dev)
    x64 = x.cpu().numpy().astype(np.float64)
    sizes = [8, 8, 3, 256, 1, 5, 100, 13, 630]
    assert sum(sizes) == 1024
    runs = []
    for _ in range(2):
        st = FeatureStats(capture_mean_cov=True)
        pos = 0
        for n in sizes:
            st.append_torch(x[pos:pos + n]); pos += n
        assert st.num_items == 1024 and st.raw_mean.is_cuda and st.raw_cov.dtype == torch.float64
        runs.append((st.raw_mean.clone(), st.raw_cov.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), 'the same batches gave other bits'
    bc, bm = _bound(x64)
    dm = np.abs(runs[0][0].cpu().numpy() - x64.sum(0)); dc = np.abs(runs[0][1].cpu().numpy() - x64.T @ x64)
    print(f'raw_mean worst |delta| / bound {np.max(dm / bm):.3e}; raw_cov worst |delta| / bound {np.max(dc / bc):.3e}')
    assert (dm <= bm).all() and (dc <= bc).all()
    mean, cov = st.get_mean_cov()
    assert np.allclose(mean, x64.mean(0), rtol=1e-12, atol=0) and np.allclose(cov, np.cov(x64.T, bias=True), rtol=1e-9, atol=1e-12)
    # max_items reached in the middle of a batch: exactly max_items rows are counted
    st = FeatureStats(capture_mean_cov=True, capture_all=True, max_items=21)
    for i in range(0, 40, 8):
        st.append_torch(x[i:i + 8])
    assert st.num_items == 21 and st.is_full() and st.get_all().shape == (21, 256)
    y64 = x64[:21]
    bc, bm = _bound(y64)
    assert (np.abs(st.raw_mean.cpu().numpy() - y64.sum(0)) <= bm).all() and (np.abs(st.raw_cov.cpu().numpy() - y64.T @ y64) <= bc).all()


def test_fid_from_gpu_features_matches_the_reference(dev):
    """Cases A (1024 vs 1024) and B (the first 96 of each, singular covariances): GPU features -> FeatureStats -> frechet_distance against the
    reference's FeatureStats + scipy.linalg.sqrtm value, |delta| <= 10 x the stored shift of the case.  The fixture's shifts (how far the
    reference's own value moves when its features move by 2e-5 relative, or the eigenvalue form from the sqrtm form, whichever is larger):
    A 1.19e-06 (2.4e-06 relative, FID 0.48728), B 2.47e-06 (4.9e-07 relative, FID 4.99769)."""
    from layoutdetr_amd.metrics.layout_frechet_inception_distance import frechet_distance
    from layoutdetr_amd.metrics.metric_utils_layout import FeatureStats
    net = _net(dev)
    f = [_fused(net, *_to(dev, C.seeded_layouts(tag))) for tag in ('real', 'fake')]
    for case, n in (('A', 1024), ('B', 96)):
        mc = []
        for feat in f:
            st = FeatureStats(capture_mean_cov=True, max_items=n)
            for i in range(0, n, 8):
                st.append_torch(feat[i:i + 8])
            mc.append(st.get_mean_cov())
        got = frechet_distance(*mc[1], *mc[0])
        want, shift = float(GOLD[f'fid_{case}']), float(GOLD[f'fid_{case}_shift'])
        print(f'FID case {case}: {got!r} vs {want!r}: |delta| {abs(got - want):.3e}, bar {10 * shift:.3e}')
        assert abs(got - want) <= 10 * shift


def test_the_four_means_match_the_reference(dev):
    from layoutdetr_amd.metrics.metric_layoutnet import compute_alignment, compute_overlap
    from layoutdetr_amd.metrics.overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k import layoutwise_means
    real, fake = _to(dev, C.seeded_layouts('real')), _to(dev, C.seeded_layouts('fake'))
    mask = ~real[2]
    iou, docsim = layoutwise_means(real[0], fake[0], mask)
    got = [compute_overlap(fake[0], mask).mean().item(), compute_alignment(fake[0], mask).mean().item(), iou.mean().item(), docsim.mean().item()]
    for name, g, w in zip(MEANS, got, GOLD['means_seeded'].tolist()):
        print(f'{name}: {g!r} vs {w!r} ({abs(g - w) / abs(w):.2e})')
        assert abs(g - w) <= 1e-5 * abs(w), name


def _case_c_kwargs(tmp_path, monkeypatch, dev):
    from layoutdetr_amd.training.networks_layoutnet import LayoutNet
    zpath = C.stage_dataset(tmp_path)
    C.write_detector(tmp_path, LayoutNet)
    monkeypatch.chdir(tmp_path)
    return dict(G=C.StubGenerator().to(dev), dataset_kwargs=dict(class_name='layoutdetr_amd.training.dataset_layoutganpp.LayoutDataset', path=zpath, use_labels=False,
                                                                  max_size=None, xflip=False, background_size=32), num_gpus=1, rank=0, device=dev)


def test_calc_metric_reproduces_the_reference_end_to_end(dev, tmp_path, monkeypatch):
    """Case C: the tiny archive (3 items: a singular covariance on purpose), the stub generator, the label map on the path.  FID within
    10 x the case's shift (fixture: 5.36e-05, 2.9e-06 relative, FID 18.52048), the four means to 1e-5 relative."""
    from layoutdetr_amd.metrics import metric_main
    kw = _case_c_kwargs(tmp_path, monkeypatch, dev)
    run_dir = tmp_path / 'run'
    run_dir.mkdir()
    r = metric_main.calc_metric(FID_NAME, cache=False, **kw)
    want, shift = float(GOLD['C_fid']), float(GOLD['fid_C_shift'])
    print(f'case C FID {r.results[FID_NAME]!r} vs {want!r}: |delta| {abs(r.results[FID_NAME] - want):.3e}, bar {10 * shift:.3e}')
    assert abs(r.results[FID_NAME] - want) <= 10 * shift
    assert not (tmp_path / 'metric-cache').exists() and r.metric == FID_NAME and r.num_gpus == 1
    m = metric_main.calc_metric(MEANS_NAME, cache=False, **kw)
    for name, w in zip(MEANS, GOLD['C_means'].tolist()):
        print(f'{name}: {m.results[name]!r} vs {w!r}')
        assert abs(m.results[name] - w) <= 1e-5 * abs(w), name
    for res in (r, m):
        metric_main.report_metric(res, run_dir=str(run_dir), snapshot_pkl=str(run_dir / 'network-snapshot-000000.pkl'))
        lines = open(run_dir / f'metric-{res.metric}.jsonl').read().splitlines()
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d['metric'] == res.metric and d['results'] == dict(res.results) and d['snapshot_pkl'] == 'network-snapshot-000000.pkl'
    # the real-data statistics are cached below cache_dir only, and a second call reads them: the same bits
    cache = tmp_path / 'cache'
    a = metric_main.calc_metric(FID_NAME, cache_dir=str(cache), **kw)
    files = list(cache.iterdir())
    assert len(files) == 1 and files[0].suffix == '.pkl'
    from layoutdetr_amd.metrics import metric_utils_layout as mu
    calls = []
    real_extract = mu.get_feature_detector

    def counting(*args, **kwargs):
        calls.append(1)
        return real_extract(*args, **kwargs)
    monkeypatch.setattr(mu, 'get_feature_detector', counting)
    b = metric_main.calc_metric(FID_NAME, cache_dir=str(cache), **kw)
    assert len(calls) == 1, 'the dataset pass ran again although its statistics were cached'
    assert a.results[FID_NAME] == b.results[FID_NAME] == r.results[FID_NAME]


def _training_kwargs(tmp_path, zpath, metrics):
    words = set()
    import zipfile
    with zipfile.ZipFile(zpath) as z:
        for s in json.loads(z.read('non_image.json'))['samples']:
            for t in s[1]['texts']:
                words.update(t.replace('%', ' % ').replace('!', ' !').split())
    vf = tmp_path / 'vocab.txt'
    vf.write_text('\n'.join(['[PAD]', '[unused0]', '[UNK]', '[CLS]', '[SEP]', '[MASK]'] + sorted(words)) + '\n')
    net = dict(bert_f_dim=768, bert_num_heads=4, bert_num_encoder_layers=2, bert_num_decoder_layers=2, im_f_dim=512, text_mode='encoder', tokenizer_vocab=str(vf))
    ds = dict(class_name='training.dataset_layoutganpp.LayoutDataset', path=zpath, use_labels=False, max_size=3, xflip=False, background_size=64)
    return dict(
        training_set_kwargs=ds, validation_set_kwargs=dict(ds), metrics=metrics,
        data_loader_kwargs=dict(num_workers=0), random_seed=0, num_gpus=1, rank=0, batch_size=2, batch_gpu=2,
        G_kwargs=dict(class_name='training.networks_detr.Generator', z_dim=4, **net), D_kwargs=dict(class_name='training.networks_detr.Discriminator', **net),
        G_opt_kwargs=dict(class_name='torch.optim.Adam', betas=[0, 0.99], eps=1e-8, lr=1e-5), D_opt_kwargs=dict(class_name='torch.optim.Adam', betas=[0, 0.99], eps=1e-8, lr=1e-5),
        loss_kwargs=dict(class_name='training.loss.StyleGAN2Loss', r1_gamma=0.0, pl_weight=0.0), G_reg_interval=4, D_reg_interval=16,
        ema_kimg=2 * 10 / 32, total_kimg=0.006, kimg_per_tick=0.002, network_snapshot_ticks=2)


def test_training_loop_evaluates_the_registered_metrics(dev, tmp_path, monkeypatch, capsys):
    import importlib
    from layoutdetr_amd import dropin
    from layoutdetr_amd.metrics import metric_main
    from layoutdetr_amd.training.networks_layoutnet import LayoutNet
    zpath = C.stage_dataset(tmp_path)
    C.write_detector(tmp_path, LayoutNet)
    monkeypatch.chdir(tmp_path)
    run_dir = tmp_path / 'run'
    run_dir.mkdir()
    names = metric_main.list_valid_metrics()
    assert len(names) == 4
    dropin.install()
    try:
        tl = importlib.import_module('training.training_loop')
        out = tl.training_loop(run_dir=str(run_dir), **_training_kwargs(tmp_path, zpath, names + ['fid50k_full']))
        text = capsys.readouterr().out
        assert text.count('fid50k_full') == 1 and 'not registered' in text
        keys = ['layout_fid50k_train', 'layout_fid50k_val'] + list(MEANS) + [k.replace('_train', '_val') for k in MEANS]
        for k in keys:
            assert np.isfinite(out['metrics'][k]) and out['stats'][f'Metrics/{k}'] == out['metrics'][k], k
        assert not any('fid50k_full' in k for k in out['metrics'])
        for n in names:
            lines = open(run_dir / f'metric-{n}.jsonl').read().splitlines()
            assert len(lines) >= 1 and all(json.loads(l)['metric'] == n for l in lines)
        assert not (run_dir / 'metric-fid50k_full.jsonl').exists()
        logged = [json.loads(l) for l in open(run_dir / 'stats.jsonl').read().splitlines()]
        with_metrics = [d for d in logged if any(k.startswith('Metrics/') for k in d)]
        assert with_metrics and all(f'Metrics/{k}' in with_metrics[-1] and np.isfinite(with_metrics[-1][f'Metrics/{k}']['mean']) for k in keys)
        assert (run_dir / 'metric-cache').is_dir()
        # one direct evaluation: G_ema bit-identical afterwards, torch's CPU and GPU generator states as they were found
        G_ema = out['G_ema']
        before = {k: v.detach().clone() for k, v in list(G_ema.named_parameters()) + list(G_ema.named_buffers())}
        mode = G_ema.training
        torch.manual_seed(123)
        cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
        ds = dict(_training_kwargs(tmp_path, zpath, [])['training_set_kwargs'])
        r = metric_main.calc_metric(FID_NAME, G=G_ema, dataset_kwargs=ds, num_gpus=1, rank=0, device=dev, cache=False)
        assert np.isfinite(r.results[FID_NAME]) and G_ema.training == mode
        after = dict(list(G_ema.named_parameters()) + list(G_ema.named_buffers()))
        assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before), 'an evaluation changed G_ema'
        assert torch.equal(torch.get_rng_state(), cpu_state), 'an evaluation moved the CPU generator'
        assert torch.equal(torch.cuda.get_rng_state(dev), gpu_state), 'an evaluation moved the GPU generator (gen_z is drawn from it)'
    finally:
        dropin.uninstall()


_TWO_RANK = r'''
import os, sys, json, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["LDETR_ROOT"]); sys.path.insert(0, os.path.join(os.environ["LDETR_ROOT"], "tests"))
import layout_eval_common as C
from layoutdetr_amd.metrics import metric_main, metric_utils_layout as mu
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0); dev = torch.device("cuda", 0)
if world > 1:
    dist.init_process_group("gloo")
os.chdir(os.environ["LDETR_TMP"])
zpath = os.path.join(os.environ["LDETR_TMP"], C.DATASET_NAME, "zip", "train.zip")
kw = dict(G=C.StubGenerator().to(dev), dataset_kwargs=dict(class_name="layoutdetr_amd.training.dataset_layoutganpp.LayoutDataset", path=zpath, use_labels=False,
          max_size=None, xflip=False, background_size=32), num_gpus=world, rank=rank, device=dev, cache=False)
opts = mu.MetricOptions(**kw)
walk = mu._ItemWalk(opts, mu._construct(opts.dataset_kwargs), None, None, dict(num_workers=0))
kept = [(len(s["name"]), real) for s, _l, real in walk]
st = mu.compute_feature_stats_for_generator(opts=opts, detector_pth="pretrained/layoutnet_%s.pth.tar" % C.DATASET_NAME, detector_kwargs={}, capture_mean_cov=True, capture_all=True, max_items=50000)
fid = metric_main.calc_metric("layout_fid50k_train", **kw).results["layout_fid50k_train"]
means = metric_main.calc_metric("overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k_train", **kw).results
np.savez(os.environ["LDETR_OUT"] + f".{world}.{rank}.npz", raw_mean=st.raw_mean.cpu().numpy(), raw_cov=st.raw_cov.cpu().numpy(), num_items=st.num_items, fid=fid, all=st.get_all(),
         subset=np.array(walk.item_subset), kept=json.dumps(kept), means=np.array([means[k] for k in sorted(means)]))
if world > 1:
    dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_combine_their_shares(dev, tmp_path):
    """World 2 over gloo, both ranks on device 0, case C's 3-item dataset: rank 0 walks items [0, 2], rank 1 walks [1, 0] -- its second item is a
    wrapped repeat and is skipped.  The combined raw sums equal the single-rank ones within the float64 bound of the statistics test; the FID
    within 10 x the case's shift of the reference value; both ranks return the broadcast value."""
    from layoutdetr_amd.training.networks_layoutnet import LayoutNet
    C.stage_dataset(tmp_path)
    C.write_detector(tmp_path, LayoutNet)
    out = str(tmp_path / 'res')
    env = dict(os.environ, LDETR_ROOT=ROOT, LDETR_TMP=str(tmp_path), LDETR_OUT=out, HSA_ENABLE_IPC_MODE_LEGACY='0')
    subprocess.check_call([sys.executable, '-c', _TWO_RANK], env=dict(env, RANK='0', WORLD_SIZE='1'), timeout=600)
    subprocess.check_call([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                           '--master-port', '29541', '--no-python', sys.executable, '-c', _TWO_RANK], env=env, timeout=600)
    one = np.load(out + '.1.0.npz')
    two = [np.load(out + f'.2.{r}.npz') for r in range(2)]
    assert two[0]['subset'].tolist() == [0, 2] and two[1]['subset'].tolist() == [1, 0]
    assert json.loads(str(two[0]['kept'])) == [[2, None]] and json.loads(str(two[1]['kept'])) == [[2, [0]]], 'rank 1 must drop its wrapped second item'
    want, shift = float(GOLD['C_fid']), float(GOLD['fid_C_shift'])
    for t in two:
        assert int(t['num_items']) == int(one['num_items']) == 3
        assert t['all'].shape == (3, 256) and np.array_equal(t['all'], one['all']), 'the gathered features are not in dataset order'
        bc, bm = _bound(one['all'].astype(np.float64))
        assert (np.abs(t['raw_mean'] - one['raw_mean']) <= bm).all() and (np.abs(t['raw_cov'] - one['raw_cov']) <= bc).all()
        print(f'two-rank FID {float(t["fid"])!r}, one-rank {float(one["fid"])!r}, reference {want!r}, bar {10 * shift:.3e}')
        assert abs(float(t['fid']) - want) <= 10 * shift
        assert np.allclose(t['means'], one['means'], rtol=1e-6, atol=0)
    assert float(two[0]['fid']) == float(two[1]['fid']) and np.array_equal(two[0]['means'], two[1]['means'])
