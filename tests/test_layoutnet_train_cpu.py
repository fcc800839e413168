"""Training the layout-FID detector, without a GPU: the float restatement of LayoutNet.forward and of the detector's loss
(tests/layoutnet_train_common.py) against the reference's values (tests/golden/layoutnet_train.npz, tools/gen_layoutnet_train_golden.py), the
trainer's pure functions, LayoutDataset.layouts(), the output-path / label-count rule, the command line and the argument checks of the new
device entry point."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import layout_eval_common as C
import layoutnet_train_common as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'layoutnet_train.npz'), allow_pickle=False)
FEATURE_TOL = 2e-5


def _rel(got, want):
    want = torch.as_tensor(want).double()
    return ((got.detach().double() - want).abs().max() / want.abs().max()).item()


def _state(num_label, dtype):
    from layoutdetr_amd.training.networks_layoutnet import LayoutNet
    return T.to_dtype(C.seeded_layoutnet_state(LayoutNet(num_label)), dtype)


@pytest.mark.parametrize('tag', sorted(T.CASES))
def test_restatement_matches_the_reference_forward_and_loss(tag):
    """float64 within 1e-10 of the reference's float64 run, float32 within FEATURE_TOL of it (the reference's own float32 run is 1.8e-6 away)."""
    bbox, label, pad, is_real = T.case_inputs(tag)
    for dtype, suffix, tol in ((torch.float64, 'f64', 1e-10), (torch.float32, 'f64', FEATURE_TOL)):
        sd = _state(T.CASES[tag]['num_label'], dtype)
        disc, cls, box, _ = T.forward_ref(sd, bbox.to(dtype), label, pad)
        for key, got in (('disc', disc), ('cls', cls), ('box', box)):
            want = GOLD[f'{tag}_{key}_{suffix}']
            assert tuple(got.shape) == want.shape
            e = _rel(got, want)
            print(tag, dtype, key, f'{e:.3e}')
            assert e <= tol, (tag, dtype, key, e)
        if dtype == torch.float64:
            terms = T.loss_terms(disc, cls, box, bbox, label, pad, is_real)[:3]
            for got, want in zip(terms, GOLD[f'{tag}_loss_terms']):
                assert abs(got.item() - want) <= 1e-10 * abs(want), (tag, got.item(), want)


def test_perturb_and_the_trajectory_batches():
    from layoutdetr_amd.train_layoutnet import perturb
    batches = T.trajectory_batches()
    assert len(batches) == T.TRAJ['steps']
    assert torch.equal(batches[0][0], torch.from_numpy(GOLD['traj_batch0_bbox'])) and torch.equal(batches[0][3], torch.from_numpy(GOLD['traj_batch0_is_real']))
    bbox, _, _ = C.seeded_layouts('train.traj', n=16, N=9)
    flags = torch.arange(16) % 3 == 0
    eps = torch.linspace(-60, 60, 16 * 9 * 4).reshape(16, 9, 4)      # large enough that both clamps act
    got = perturb(bbox, flags, eps, 0.01)
    assert torch.equal(got, T.perturb_ref(bbox, flags, eps, 0.01))
    assert torch.equal(got[~flags], bbox[~flags]) and not torch.equal(got[flags], bbox[flags])
    assert got.min() >= 0.0 and got.max() <= 1.0 and (got == 0.0).any() and (got == 1.0).any()
    # the stored trajectory is a training run: the reference's loss falls
    tot = GOLD['traj_losses_f64'][:, 3]
    assert tot.shape == (8,) and tot[-1] < tot[0]
    assert np.allclose(GOLD['traj_losses_f64'][:, 0] + GOLD['traj_losses_f64'][:, 1] + T.W_BBOX * GOLD['traj_losses_f64'][:, 2], tot, rtol=1e-12)


def test_layouts_equal_the_item_fields_without_decoding_an_image(tmp_path, monkeypatch):
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset
    zpath = C.stage_dataset(tmp_path)
    ds = LayoutDataset(path=zpath, background_size=32)
    items = [ds[i][0] for i in range(len(ds))]

    def no_decode(self, fname):
        raise AssertionError(f'layouts() decoded {fname}')
    monkeypatch.setattr(LayoutDataset, '_decode', no_decode)
    bboxes, labels, mask = ds.layouts()
    n = len(ds)
    assert bboxes.shape == (n, 9, 4) and bboxes.dtype == torch.float32 and labels.shape == (n, 9) and labels.dtype == torch.int64
    assert mask.shape == (n, 9) and mask.dtype == torch.bool
    for i, it in enumerate(items):
        assert np.array_equal(bboxes[i].numpy(), it['bboxes']) and np.array_equal(labels[i].numpy(), it['labels']) and np.array_equal(mask[i].numpy(), it['mask'])
    sub = LayoutDataset(path=zpath, background_size=32, max_size=2)
    assert len(sub) == 2
    b2, l2, m2 = sub.layouts()
    idx = torch.from_numpy(sub._raw_idx)
    assert torch.equal(b2, bboxes[idx]) and torch.equal(l2, labels[idx]) and torch.equal(m2, mask[idx])


def test_output_path_and_label_count_follow_the_metric():
    from layoutdetr_amd import train_layoutnet as tn
    from layoutdetr_amd.metrics import metric_layoutnet as ml
    assert tn.detector_path('ads_banner_collection') == 'pretrained/layoutnet_ads_banner_collection.pth.tar'
    for name in ('rico', 'enrico', 'clay', 'ads_banner_collection', 'AMT_uploaded_ads_banners', 'cgl_dataset'):
        assert ml.detector_num_label(tn.detector_path(name)) == 13
    assert ml.detector_num_label(tn.detector_path('my_banners')) == 5 and ml.detector_num_label('pretrained/layoutnet_tests.pth.tar') == 5
    lab = torch.tensor([[0, 5, 6, 7], [1, 2, 3, 4]])
    mask = torch.ones(2, 4, dtype=torch.bool)
    # ads_banner_collection: 13 labels and the label_idx_replace table
    mapped, n = tn.prepare_labels(lab, mask, tn.detector_path('ads_banner_collection'))
    assert n == 13 and mapped.tolist() == [[2, 4, 7, 3], [2, 2, 2, 2]]
    # cgl_dataset: label_idx_replace_2
    mapped, n = tn.prepare_labels(lab[1:] % 5, mask[1:], tn.detector_path('cgl_dataset'))
    assert n == 13 and mapped.tolist() == [[2, 4, 3, 2]]
    # an 8-label archive under a name the reference does not list: 5 labels, no relabelling -> refused, naming the rule
    with pytest.raises(ValueError, match='13 labels when the path names one of the datasets the reference lists, else 5'):
        tn.prepare_labels(lab, mask, tn.detector_path('my_banners'))
    # ... unless the offending labels sit in padded slots only
    mask2 = mask.clone(); mask2[0, 1:] = False
    mapped, n = tn.prepare_labels(lab, mask2, tn.detector_path('my_banners'))
    assert n == 5 and torch.equal(mapped, lab)


def test_command_line():
    from layoutdetr_amd import train_layoutnet as tn
    a = tn.parse_args(['--data', 'x/ds/zip/train.zip'])
    assert (a.data, a.val, a.out, a.batch, a.noise_std, a.noise_p, a.seed, a.w_bbox) == ('x/ds/zip/train.zip', None, None, 64, 0.01, 0.5, 0, 10.0)
    a = tn.parse_args(['--data', 'a.zip', '--val', 'b.zip', '--out', 'o.pth.tar', '--steps', '7', '--batch', '8', '--lr', '3e-4', '--beta1', '0.5', '--dropout', '0',
                       '--noise-std', '0.02', '--noise-p', '0.25', '--seed', '3', '--eval-every', '2', '--max-size', '10', '--w-bbox', '1'])
    assert (a.val, a.out, a.steps, a.batch, a.lr, a.beta1, a.dropout, a.noise_std, a.noise_p, a.seed, a.eval_every, a.max_size, a.w_bbox) == \
        ('b.zip', 'o.pth.tar', 7, 8, 3e-4, 0.5, 0.0, 0.02, 0.25, 3, 2, 10, 1.0)
    with pytest.raises(SystemExit):
        tn.parse_args([])


def test_forward_entry_point_is_declared_and_validates_before_launching():
    from layoutdetr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ldetr_hip.h')).read()
    declared = set(re.findall(r'^\s*int\s+(ldetr_\w+)\s*\(', hdr, flags=re.M))
    assert 'ldetr_layoutnet_forward_f32' in declared and 'ldetr_layoutnet_forward_f32' in _lib.SIGNATURES
    assert 'networks_layoutnet.py:68-86' in hdr
    assert _lib.ABI_VERSION == 25        # additive entry
    lib = _lib.load()
    f = lib.ldetr_layoutnet_forward_f32
    P = ctypes.c_void_p
    ne, nd = 13 * 256 + 1453312, 1473060
    ok = dict(bbox=P(64), label=P(64), pad=P(64), enc=P(64), ne=ne, dec=P(64), nd=nd, L=13, B=1, N=9, disc=P(64), cls=P(64), box=P(64), feat=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['bbox'], a['label'], a['pad'], a['enc'], a['ne'], a['dec'], a['nd'], a['L'], a['B'], a['N'], a['disc'], a['cls'], a['box'], a['feat'], None)
    for kw, msg in ((dict(bbox=None), b'non-null'), (dict(dec=None), b'non-null'), (dict(cls=None), b'non-null'), (dict(N=16), b'at most 15 elements'),
                    (dict(ne=ne - 1), b'packed encoder weights'), (dict(nd=nd + 4), b'packed decoder weights'), (dict(L=17, ne=17 * 256 + 1453312), b'16-column tile'),
                    (dict(N=0), b'bad shape')):
        rc = call(**kw)
        assert rc != 0 and msg in lib.ldetr_last_error(), (kw, lib.ldetr_last_error())
    assert call(B=0) == 0      # empty batch: nothing is launched


def test_forward_has_no_cpu_path_and_packs_the_decoder():
    from layoutdetr_amd.training import networks_layoutnet as nl
    net = nl.LayoutNet(5)
    args = (torch.zeros(1, 2, 4), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match='no CPU path'):
        net(*args)
    with pytest.raises(NotImplementedError, match='no CPU path'):
        net.forward_dense(*args)
    assert set(nl.PATH_RUNS) == {'fused', 'composed', 'forward_fused', 'forward_composed'}
    # the second pack: the header's length whatever the label count, heads zero-padded to 16 rows, rebuilt after invalidate_packs()
    wd = net._packed_decoder()
    assert wd.numel() == 1473060 and net._packed_weights().numel() == 5 * 256 + 1453312
    cls_w = wd[1473060 - 260 - 2 * (16 * 256 + 16):][:16 * 256].reshape(16, 256)
    assert torch.equal(cls_w[:5], net.fc_out_cls.weight.detach()) and not cls_w[5:].any()
    assert torch.equal(wd[-260:-4], net.fc_out_disc.weight.detach().reshape(-1)) and wd[-4] == net.fc_out_disc.bias.detach()[0] and not wd[-3:].any()
    assert torch.equal(wd[:50 * 256], net.pos_token.detach().reshape(-1))
    assert net._packed_decoder() is wd
    net.invalidate_packs()
    assert net._packed_decoder() is not wd
