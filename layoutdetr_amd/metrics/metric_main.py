"""The metric registry and driver (reference: metrics/metric_main.py:32-112).  Registered here: the layout metrics.  The reference's image
metrics (fid50k_*, kid*, pr*, ppl*, eq*, is50k, rendering_*) need Inception pickles or a browser and are not part of this package;
training_loop() skips a name that is not registered, with a note."""
import json
import os
import time

import torch

from . import layout_frechet_inception_distance
from . import metric_utils_layout
from . import overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k

#----------------------------------------------------------------------------

_metric_dict = dict() # name => fn

def register_metric(fn):
    assert callable(fn)
    _metric_dict[fn.__name__] = fn
    return fn

def is_valid_metric(metric):
    return metric in _metric_dict

def list_valid_metrics():
    return list(_metric_dict.keys())

#----------------------------------------------------------------------------

def calc_metric(metric, **kwargs): # See metric_utils_layout.MetricOptions for the full list of arguments.
    assert is_valid_metric(metric)
    opts = metric_utils_layout.MetricOptions(**kwargs)

    # Calculate.  The passes draw gen_z from the device generator (as the reference does) and may draw labels from numpy's: the states found
    # are put back, so that whatever runs next (training) does not depend on whether a metric was evaluated.
    import numpy as np
    on_gpu = torch.device(opts.device).type == 'cuda'
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(opts.device) if on_gpu else None, np.random.get_state())
    start_time = time.time()
    try:
        results = _metric_dict[metric](opts)
    finally:
        torch.set_rng_state(rng[0])
        if on_gpu:
            torch.cuda.set_rng_state(rng[1], opts.device)
        np.random.set_state(rng[2])
    total_time = time.time() - start_time

    # Broadcast results.
    for key, value in list(results.items()):
        if opts.num_gpus > 1:
            value = torch.as_tensor(value, dtype=torch.float64, device=opts.device)
            torch.distributed.broadcast(tensor=value, src=0)
            value = float(value.cpu())
        results[key] = value

    # Decorate with metadata.
    return metric_utils_layout.EasyDict(
        results         = metric_utils_layout.EasyDict(results),
        metric          = metric,
        total_time      = total_time,
        total_time_str  = metric_utils_layout.format_time(total_time),
        num_gpus        = opts.num_gpus,
        background_filter = opts.background_filter,
    )

#----------------------------------------------------------------------------

def report_metric(result_dict, run_dir=None, snapshot_pkl=None):
    metric = result_dict['metric']
    assert is_valid_metric(metric)
    if run_dir is not None and snapshot_pkl is not None:
        snapshot_pkl = os.path.relpath(snapshot_pkl, run_dir)

    jsonl_line = json.dumps(dict(result_dict, snapshot_pkl=snapshot_pkl, timestamp=time.time()))
    print(jsonl_line)
    if run_dir is not None and os.path.isdir(run_dir):
        with open(os.path.join(run_dir, f'metric-{metric}.jsonl'), 'at') as f:
            f.write(jsonl_line + '\n')

#----------------------------------------------------------------------------

def _layout_fid(opts):
    opts.dataset_kwargs.update(max_size=None, xflip=False)
    return layout_frechet_inception_distance.compute_layout_fid(opts, max_real=None, num_gen=50000)

def _layout_means(opts):
    opts.dataset_kwargs.update(max_size=None, xflip=False)
    return overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k.compute_overlap_alignment_laywise_IoU_layerwise_DocSim(opts, max_real=None, num_gen=50000)

@register_metric
def layout_fid50k_train(opts):
    return dict(layout_fid50k_train=_layout_fid(opts))

@register_metric
def layout_fid50k_val(opts):
    return dict(layout_fid50k_val=_layout_fid(opts))

@register_metric
def overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k_train(opts):
    overlap, alignment, layoutwiseIoU, layoutwiseDocSim = _layout_means(opts)
    return dict(overlap_50k_train=overlap, alignment_50k_train=alignment, layoutwise_iou50k_train=layoutwiseIoU, layoutwise_docsim50k_train=layoutwiseDocSim)

@register_metric
def overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k_val(opts):
    overlap, alignment, layoutwiseIoU, layoutwiseDocSim = _layout_means(opts)
    return dict(overlap_50k_val=overlap, alignment_50k_val=alignment, layoutwise_iou50k_val=layoutwiseIoU, layoutwise_docsim50k_val=layoutwiseDocSim)

#----------------------------------------------------------------------------
