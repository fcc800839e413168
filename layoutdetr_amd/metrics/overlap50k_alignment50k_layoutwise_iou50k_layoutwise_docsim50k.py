"""Means of overlap, alignment, layout-wise IoU and layout-wise DocSim of the generator's boxes against the dataset's
(reference: metrics/overlap50k_alignment50k_layoutwise_iou50k_layoutwise_docsim50k.py:20-45).  The per-item values stay on the device in float32
and are averaged once; the reference scores one layout at a time on the host (:36-44) -- the per-layout means over the valid boxes are the same
numbers (the reference's np.bool, gone from current numpy, is plain bool here)."""
import torch

from . import metric_utils_layout
from .metric_layoutnet import compute_docsim_weight, compute_iou

#----------------------------------------------------------------------------

def layoutwise_means(bbox_real, bbox_fake, mask):
    """[n, N, 4] x [n, N, 4] float32, mask [n, N] bool (True = a box) -> (IoU, DocSim weight) of corresponding boxes averaged over each layout's
    boxes: compute_iou_for_layout / compute_docsim_for_layout (metric_layoutnet.py) for every layout at once, [n] float32 each."""
    n, N, _ = bbox_real.shape
    cnt = mask.to(torch.float32).sum(-1)
    out = []
    for fn in (compute_iou, compute_docsim_weight):
        v = fn(bbox_real.reshape(n * N, 4).to(torch.float32), bbox_fake.reshape(n * N, 4).to(torch.float32)).reshape(n, N)
        out.append(torch.where(mask, v, torch.zeros_like(v)).sum(-1) / cnt)
    return out[0], out[1]


def compute_overlap_alignment_laywise_IoU_layerwise_DocSim(opts, max_real, num_gen):
    stats_bbox_real, stats_bbox_fake, stats_bbox_class, stats_mask, stats_overlap, stats_alignment = metric_utils_layout.compute_maxIoU_overlap_alignment_wrapper(opts=opts, rel_lo=0, rel_hi=1, max_items=max_real)
    if opts.rank != 0:
        return float('nan'), float('nan'), float('nan'), float('nan')
    bbox_real = stats_bbox_real.get_all_torch().to(torch.float32)
    bbox_fake = stats_bbox_fake.get_all_torch().to(torch.float32)
    mask = stats_mask.get_all_torch().to(torch.bool)
    overlap = stats_overlap.get_all_torch().to(torch.float32)
    alignment = stats_alignment.get_all_torch().to(torch.float32)
    iou, docsim = layoutwise_means(bbox_real, bbox_fake, mask)
    means = torch.stack([overlap.mean(), alignment.mean(), iou.mean(), docsim.mean()]).cpu()      # the pass's one trip to the host
    return tuple(float(v) for v in means)

#----------------------------------------------------------------------------
