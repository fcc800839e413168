"""Layout metrics without a GPU: the host Fréchet distance against the reference's scipy.linalg.sqrtm form, the label maps against the reference's
in-place assignment sequences, the registry and LayoutNet's parameter surface, and the argument checks of the two device entry points
(fixture: tests/golden/layout_eval.npz, written by tools/gen_layout_eval_golden.py from the reference)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'layout_eval.npz'), allow_pickle=False)


def test_frechet_distance_matches_the_sqrtm_form():
    """Eigenvalue form against the stored scipy.linalg.sqrtm value on 64-dimensional statistics: <= 1e-10 relative at full rank, <= 1e-6 when the
    covariances are singular (20 items).  Measured on 256 dimensions: 2e-15 and 8e-10; the margin is for another LAPACK."""
    from layoutdetr_amd.metrics.layout_frechet_inception_distance import frechet_distance
    for tag, tol in (('full', 1e-10), ('deficient', 1e-6)):
        got = frechet_distance(*(GOLD[f'small_{tag}_{k}'] for k in ('mu1', 'sigma1', 'mu2', 'sigma2')))
        want = float(GOLD[f'small_{tag}_fid'])
        print(tag, got, want, abs(got - want) / abs(want))
        assert isinstance(got, float) and abs(got - want) <= tol * abs(want), (tag, got, want)
    import layoutdetr_amd.metrics.layout_frechet_inception_distance as m
    assert 'import scipy' not in open(m.__file__).read(), 'scipy must not be needed at run time'


def test_label_maps_are_the_net_effect_of_the_reference_sequences():
    from layoutdetr_amd.training import networks_layoutnet as nl
    for key, kw, table in (('map_replace', dict(label_idx_replace=True), nl.LABEL_MAP), ('map_replace2', dict(label_idx_replace_2=True), nl.LABEL_MAP_2)):
        want = torch.from_numpy(GOLD[key])
        assert len(table) == want.numel()
        lab = torch.arange(want.numel()).reshape(1, -1)
        keep = lab.clone()
        got = nl.map_labels(lab, **kw)
        assert torch.equal(got.reshape(-1), want), (key, got, want)
        assert torch.equal(lab, keep), 'the caller\'s labels were modified'
        assert list(table) == want.tolist()
    # labels beyond a map pass through (the reference's sequences do not touch them); no map: the same tensor
    big = torch.tensor([[8, 12, 5]])
    assert nl.map_labels(big, label_idx_replace=True).tolist() == [[8, 12, 4]]
    assert nl.map_labels(big) is big


def test_registry_and_layoutnet_surface():
    from layoutdetr_amd.metrics import metric_main
    from layoutdetr_amd.training.networks_layoutnet import LayoutNet
    names = ['layout_fid50k_train', 'layout_fid50k_val', 'overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k_train',
             'overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k_val']
    assert all(metric_main.is_valid_metric(n) for n in names) and sorted(metric_main.list_valid_metrics()) == sorted(names)
    assert not metric_main.is_valid_metric('fid50k_full')
    net = LayoutNet(13)
    sd = net.state_dict()
    assert sorted(sd) == GOLD['state_keys'].tolist()
    for k, shape in zip(GOLD['state_keys'].tolist(), GOLD['state_shapes'].tolist()):
        assert ','.join(str(s) for s in sd[k].shape) == shape, k
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 2, 4), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net.extract_features(torch.zeros(1, 2, 4), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.bool))
    # strict loading: a checkpoint of another network is refused loudly
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in sd.items() if not k.startswith('dec_transformer')}, strict=True)
    from layoutdetr_amd import dropin
    assert 'metrics.metric_main' not in dropin._ALIASES


def test_device_entry_points_are_declared_and_validate_before_launching():
    from layoutdetr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ldetr_hip.h')).read()
    declared = set(re.findall(r'^\s*int\s+(ldetr_\w+)\s*\(', hdr, flags=re.M))
    for name in ('ldetr_layoutnet_features_f32', 'ldetr_feature_stats_f64'):
        assert name in declared and name in _lib.SIGNATURES
    lib = _lib.load()
    P = ctypes.c_void_p
    nw = 13 * 256 + 1453312
    rc = lib.ldetr_layoutnet_features_f32(None, None, None, None, 0, None, nw, 13, 1, 9, None, None)
    assert rc != 0 and b'non-null' in lib.ldetr_last_error()
    rc = lib.ldetr_layoutnet_features_f32(P(64), P(64), P(64), None, 0, P(64), nw, 13, 1, 16, P(64), None)
    assert rc != 0 and b'at most 15 elements' in lib.ldetr_last_error()
    rc = lib.ldetr_layoutnet_features_f32(P(64), P(64), P(64), None, 0, P(64), nw - 1, 13, 1, 9, P(64), None)
    assert rc != 0 and b'packed weights' in lib.ldetr_last_error()
    bad_map = (ctypes.c_int * 16)(2, 2, 13)
    rc = lib.ldetr_layoutnet_features_f32(P(64), P(64), P(64), bad_map, 3, P(64), nw, 13, 1, 9, P(64), None)
    assert rc != 0 and b'outside the embedding table' in lib.ldetr_last_error()
    assert lib.ldetr_layoutnet_features_f32(P(64), P(64), P(64), None, 0, P(64), nw, 13, 0, 9, P(64), None) == 0      # empty batch
    rc = lib.ldetr_feature_stats_f64(None, 8, 256, None, None, None)
    assert rc != 0 and b'non-null' in lib.ldetr_last_error()
    rc = lib.ldetr_feature_stats_f64(P(64), 8, 250, P(64), P(64), None)
    assert rc != 0 and b'multiple of 16' in lib.ldetr_last_error()
    assert lib.ldetr_feature_stats_f64(P(64), 0, 256, P(64), P(64), None) == 0
