"""Feature statistics and the passes over the dataset / the generator behind the layout metrics (reference: metrics/metric_utils_layout.py).
Same names and call signatures where a caller sees them.  What differs, by design:
* `FeatureStats` keeps its accumulators on the device (float64 sums by csrc/layoutnet.hip's ldetr_feature_stats_f64) and brings them to the
  host once, in get_mean_cov() / get_all(): a pass over the data does not synchronise until its end (the reference copies every batch to the
  host and multiplies there, :110-112).
* Several ranks: each rank accumulates ITS share of the items (the wrapped tail of `item_subset`, :233, is skipped) and the shares are combined
  once by `FeatureStats.reduce`; the reference broadcasts every batch from every rank (:117-123).  The set of items is the same, the order of
  the float64 sums is not.
* `G` is run as it is (eval mode, no_grad), not through a deep copy, and is left as it was found.
* The real-data statistics are cached only below `opts.cache_dir` (the reference writes to a per-user cache directory, :211)."""
import hashlib
import os
import pickle
import time
import uuid

import numpy as np
import torch

from ..hip import core

#----------------------------------------------------------------------------

class EasyDict(dict):
    """dnnlib.EasyDict: a dict whose items are attributes as well."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value

    def __delattr__(self, name):
        del self[name]


def format_time(seconds):
    """dnnlib.util.format_time."""
    s = int(np.rint(seconds))
    if s < 60:
        return f'{s}s'
    if s < 60 * 60:
        return f'{s // 60}m {s % 60:02d}s'
    if s < 24 * 60 * 60:
        return f'{s // 3600}h {(s // 60) % 60:02d}m {s % 60:02d}s'
    return f'{s // 86400}d {(s // 3600) % 24:02d}h {(s // 60) % 60:02d}m'


class MetricOptions:
    def __init__(self, G=None, G_kwargs={}, dataset_kwargs={}, num_gpus=1, rank=0, device=None, progress=None, cache=True, run_dir=None,
                 batch_size=8, cache_dir=None, data_loader_kwargs=None, background_filter=None):
        assert 0 <= rank < num_gpus
        if background_filter not in (None, 'blur', 'edge'):
            raise ValueError(f"MetricOptions: background_filter must be None, 'blur' or 'edge' (got {background_filter!r})")
        # every page the generator sees is filtered on the device before the resize (dataset_layoutganpp.filter_pages); the real-data side of a
        # metric reads boxes only and does not depend on it, so the cache of real-data statistics keeps its key
        self.background_filter = background_filter
        self.G = G
        self.G_kwargs = EasyDict(G_kwargs)
        self.dataset_kwargs = EasyDict(dataset_kwargs)
        self.num_gpus = num_gpus
        self.rank = rank
        self.device = device if device is not None else torch.device('cuda', rank)
        self.progress = progress.sub() if progress is not None and rank == 0 else ProgressMonitor()
        self.cache = cache
        self.run_dir = run_dir
        self.batch_size = batch_size
        self.data_loader_kwargs = data_loader_kwargs      # None: the passes load in-process (_ItemWalk)
        # where the real-data statistics may be cached; nothing is ever written outside it
        self.cache_dir = cache_dir if cache_dir is not None else (os.path.join(run_dir, 'metric-cache') if (cache and run_dir) else None)

#----------------------------------------------------------------------------

_feature_detector_cache = dict()

def get_feature_detector_name(pth):
    return os.path.splitext(pth.split('/')[-1])[0]

def get_feature_detector(pth, device=None, num_gpus=1, rank=0, verbose=False):
    from .metric_layoutnet import LayoutFID
    assert 0 <= rank < num_gpus
    device = torch.device(device if device is not None else 'cuda')
    key = (os.path.abspath(pth), os.path.getmtime(pth) if os.path.exists(pth) else None, str(device))
    if key not in _feature_detector_cache:
        is_leader = (rank == 0)
        if not is_leader and num_gpus > 1:
            torch.distributed.barrier() # leader goes first
        _feature_detector_cache[key] = LayoutFID(pth, device)
        if is_leader and num_gpus > 1:
            torch.distributed.barrier() # others follow
    return _feature_detector_cache[key]

#----------------------------------------------------------------------------

def iterate_random_labels(opts, batch_size):
    if opts.G.c_dim == 0:
        c = torch.zeros([batch_size, opts.G.c_dim], device=opts.device)
        while True:
            yield c
    else:
        dataset = _construct(opts.dataset_kwargs)
        while True:
            c = [dataset.get_label(np.random.randint(len(dataset))) for _i in range(batch_size)]
            yield torch.from_numpy(np.stack(c)).to(opts.device)

#----------------------------------------------------------------------------

def _all_gather(t):
    """torch.distributed.all_gather of equally shaped device tensors; gloo gathers host tensors only."""
    import torch.distributed as dist
    world = dist.get_world_size()
    if dist.get_backend() == 'gloo' and t.is_cuda:
        parts = [torch.empty(t.shape, dtype=t.dtype) for _ in range(world)]
        dist.all_gather(parts, t.cpu())
        return [p.to(t.device) for p in parts]
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t.contiguous())
    return parts


class FeatureStats:
    def __init__(self, capture_all=False, capture_mean_cov=False, max_items=None):
        self.capture_all = capture_all
        self.capture_mean_cov = capture_mean_cov
        self.max_items = max_items
        self.num_items = 0
        self.num_features = None
        self.all_features = None
        self.raw_mean = None
        self.raw_cov = None

    def set_num_features(self, num_features, device=None):
        if self.num_features is not None:
            assert num_features == self.num_features
        else:
            self.num_features = num_features
            self.all_features = []
            if self.capture_mean_cov:
                if num_features % 16 != 0 or not 16 <= num_features <= 256:
                    raise NotImplementedError(f'FeatureStats: mean / covariance of {num_features} features (the device kernel takes a multiple of 16 up to 256)')
                self.raw_mean = torch.zeros([num_features], dtype=torch.float64, device=device)
                self.raw_cov = torch.zeros([num_features, num_features], dtype=torch.float64, device=device)

    def is_full(self):
        return (self.max_items is not None) and (self.num_items >= self.max_items)

    def append(self, x):
        """Host array -> device -> append_torch (the reference's entry point for numpy input)."""
        self.append_torch(torch.as_tensor(np.asarray(x)).to(torch.device('cuda', torch.cuda.current_device())))

    def append_torch(self, x, num_gpus=1, rank=0):
        """The rows of x [n, ...] (a device tensor) join THIS rank's share; nothing comes to the host.  `num_gpus` / `rank` are accepted for the
        reference's signature: the ranks' shares meet in reduce(), not here."""
        assert isinstance(x, torch.Tensor)
        assert 0 <= rank < num_gpus
        core.require_gpu(x)
        if (self.max_items is not None) and (self.num_items + x.shape[0] > self.max_items):
            if self.num_items >= self.max_items:
                return
            x = x[:self.max_items - self.num_items]
        self.set_num_features(x.shape[1], device=x.device)
        self.num_items += x.shape[0]
        if self.capture_all:
            self.all_features.append(x.detach().clone())
        if self.capture_mean_cov:
            assert x.dim() == 2
            x32 = core.f32c(x.detach())
            core.check(core.lib().ldetr_feature_stats_f64(core.ptr(x32), x32.shape[0], x32.shape[1], core.ptr(self.raw_mean), core.ptr(self.raw_cov),
                                                          core.stream()), 'feature_stats')

    def reduce(self, num_gpus, rank, per_rank_items=None, total_items=None):
        """Combine the ranks' shares (every rank ends with the whole): ONE float64 SUM all-reduce of (num_items, raw_mean, raw_cov); per-item arrays by
        one all-gather, re-interleaved to dataset order (item j of the dataset sits at position j // num_gpus of rank j % num_gpus)."""
        if num_gpus <= 1:
            return self
        import torch.distributed as dist
        if self.capture_mean_cov:
            F = self.num_features
            packed = torch.cat([torch.tensor([float(self.num_items)], dtype=torch.float64, device=self.raw_mean.device), self.raw_mean, self.raw_cov.reshape(-1)])
            dist.all_reduce(packed, op=dist.ReduceOp.SUM)
            total = int(round(packed[0].item()))
            self.raw_mean, self.raw_cov = packed[1:1 + F].clone(), packed[1 + F:].reshape(F, F).clone()
        if self.capture_all:
            mine = torch.cat(self.all_features, dim=0)
            as_bool = mine.dtype == torch.bool
            if as_bool:
                mine = mine.to(torch.uint8)
            slots = per_rank_items
            pad = torch.zeros((slots,) + tuple(mine.shape[1:]), dtype=mine.dtype, device=mine.device)
            pad[:mine.shape[0]] = mine
            parts = _all_gather(pad)
            inter = torch.stack(parts, dim=1).flatten(0, 1)        # position i of rank r -> i * num_gpus + r = the dataset index
            self.all_features = [inter[:total_items].to(torch.bool) if as_bool else inter[:total_items]]
            total = total_items
        self.num_items = total
        return self

    def get_all_torch(self):
        assert self.capture_all
        return torch.cat(self.all_features, dim=0)

    def get_all(self):
        return self.get_all_torch().cpu().numpy()

    def get_mean_cov(self):
        assert self.capture_mean_cov
        raw_mean = self.raw_mean.cpu().numpy() if torch.is_tensor(self.raw_mean) else np.asarray(self.raw_mean)
        raw_cov = self.raw_cov.cpu().numpy() if torch.is_tensor(self.raw_cov) else np.asarray(self.raw_cov)
        mean = raw_mean / self.num_items
        cov = raw_cov / self.num_items
        cov = cov - np.outer(mean, mean)
        return mean, cov

    def save(self, pkl_file):
        d = dict(self.__dict__)
        for k in ('raw_mean', 'raw_cov'):
            if torch.is_tensor(d[k]):
                d[k] = d[k].cpu().numpy()
        if d['all_features'] is not None:
            d['all_features'] = [a.cpu().numpy() if torch.is_tensor(a) else a for a in d['all_features']]
        with open(pkl_file, 'wb') as f:
            pickle.dump(d, f)

    @staticmethod
    def load(pkl_file):
        with open(pkl_file, 'rb') as f:
            s = pickle.load(f)
        obj = FeatureStats(capture_all=s['capture_all'], max_items=s['max_items'])
        obj.__dict__.update(s)
        if obj.all_features is not None:
            obj.all_features = [torch.as_tensor(a) for a in obj.all_features]
        return obj

#----------------------------------------------------------------------------

class ProgressMonitor:
    def __init__(self, tag=None, num_items=None, flush_interval=1000, verbose=False, progress_fn=None, pfn_lo=0, pfn_hi=1000, pfn_total=1000):
        self.tag = tag
        self.num_items = num_items
        self.verbose = verbose
        self.flush_interval = flush_interval
        self.progress_fn = progress_fn
        self.pfn_lo = pfn_lo
        self.pfn_hi = pfn_hi
        self.pfn_total = pfn_total
        self.start_time = time.time()
        self.batch_time = self.start_time
        self.batch_items = 0
        if self.progress_fn is not None:
            self.progress_fn(self.pfn_lo, self.pfn_total)

    def update(self, cur_items):
        assert (self.num_items is None) or (cur_items <= self.num_items)
        if (cur_items < self.batch_items + self.flush_interval) and (self.num_items is None or cur_items < self.num_items):
            return
        cur_time = time.time()
        total_time = cur_time - self.start_time
        time_per_item = (cur_time - self.batch_time) / max(cur_items - self.batch_items, 1)
        if (self.verbose) and (self.tag is not None):
            print(f'{self.tag:<19s} items {cur_items:<7d} time {format_time(total_time):<12s} ms/item {time_per_item*1e3:.2f}')
        self.batch_time = cur_time
        self.batch_items = cur_items
        if (self.progress_fn is not None) and (self.num_items is not None):
            self.progress_fn(self.pfn_lo + (self.pfn_hi - self.pfn_lo) * (cur_items / self.num_items), self.pfn_total)

    def sub(self, tag=None, num_items=None, flush_interval=1000, rel_lo=0, rel_hi=1):
        return ProgressMonitor(
            tag             = tag,
            num_items       = num_items,
            flush_interval  = flush_interval,
            verbose         = self.verbose,
            progress_fn     = self.progress_fn,
            pfn_lo          = self.pfn_lo + (self.pfn_hi - self.pfn_lo) * rel_lo,
            pfn_hi          = self.pfn_lo + (self.pfn_hi - self.pfn_lo) * rel_hi,
            pfn_total       = self.pfn_total,
        )

#----------------------------------------------------------------------------

def _construct(dataset_kwargs):
    from ..training.training_loop import construct_class_by_name
    return construct_class_by_name(**dataset_kwargs)


def _label_flags(detector_pth):
    return dict(label_idx_replace='ads_banner_collection' in detector_pth or 'AMT_uploaded_ads_banners' in detector_pth,
                label_idx_replace_2='cgl_dataset' in detector_pth)


class _ItemWalk(object):
    """The items one rank visits (reference :233): positions i = 0 .. ceil(num_items / num_gpus) - 1 hold item (i * num_gpus + rank) % num_items.
    A position whose global index i * num_gpus + rank is >= num_items is a WRAPPED repeat of an early item: visited (every rank takes the same
    number of steps) and dropped from the statistics by keep()."""

    def __init__(self, opts, dataset, max_items, batch_size, data_loader_kwargs):
        self.num_items = len(dataset) if max_items is None else min(len(dataset), max_items)
        self.world, self.rank = opts.num_gpus, opts.rank
        self.per_rank = (self.num_items - 1) // self.world + 1
        self.item_subset = [(i * self.world + self.rank) % self.num_items for i in range(self.per_rank)]
        self.batch_size = batch_size if batch_size is not None else opts.batch_size
        # The reference forks three loader workers per pass (:202).  A metric pass starts in the middle of a run, from a process that has driven the GPU
        # runtime and its thread pools for a while -- forking loader workers from such a process stalled a pass in the test suite -- and an item in
        # device mode costs one PNG inflate, so the default is to load in-process; `data_loader_kwargs` (here or in MetricOptions) chooses otherwise.
        # (No pinned staging either: it would materialise the 0-stride patch placeholder, 7 MB per sample.)
        if data_loader_kwargs is None:
            data_loader_kwargs = opts.data_loader_kwargs
        kw = dict(num_workers=0) if data_loader_kwargs is None else dict(data_loader_kwargs)
        if getattr(dataset, 'mode', None) in ('device', 'raw', 'packed') and hasattr(dataset, 'collate'):
            kw.setdefault('collate_fn', dataset.collate)
        self.loader = torch.utils.data.DataLoader(dataset=dataset, sampler=self.item_subset, batch_size=self.batch_size, **kw)

    def __iter__(self):
        pos = 0
        for samples, labels in self.loader:
            n = samples['bboxes'].shape[0]
            real = [i for i in range(n) if (pos + i) * self.world + self.rank < self.num_items]
            pos += n
            yield samples, labels, (None if len(real) == n else real)


def _keep(t, real):
    return t if real is None else t[torch.as_tensor(real, dtype=torch.int64, device=t.device)]


def compute_feature_stats_for_dataset(opts, detector_pth, detector_kwargs, rel_lo=0, rel_hi=1, batch_size=None, data_loader_kwargs=None, max_items=None, **stats_kwargs):
    dataset = _construct(opts.dataset_kwargs)

    # Try to lookup from cache.
    cache_file = None
    if opts.cache and opts.cache_dir is not None:
        args = dict(dataset_kwargs=opts.dataset_kwargs, detector_pth=detector_pth, detector_kwargs=detector_kwargs, stats_kwargs=stats_kwargs, max_items=max_items)
        md5 = hashlib.md5(repr(sorted(args.items())).encode('utf-8'))
        cache_tag = f'{dataset.name}-{get_feature_detector_name(detector_pth)}-{md5.hexdigest()}'
        cache_file = os.path.join(opts.cache_dir, cache_tag + '.pkl')

        # Check if the file exists (all processes must agree).
        flag = os.path.isfile(cache_file) if opts.rank == 0 else False
        if opts.num_gpus > 1:
            flag = torch.as_tensor(flag, dtype=torch.float32, device=opts.device)
            torch.distributed.broadcast(tensor=flag, src=0)
            flag = (float(flag.cpu()) != 0)

        # Load.
        if flag:
            return FeatureStats.load(cache_file)

    # Initialize.
    walk = _ItemWalk(opts, dataset, max_items, batch_size, data_loader_kwargs)
    stats = FeatureStats(max_items=walk.num_items, **stats_kwargs)
    progress = opts.progress.sub(tag='dataset features', num_items=walk.num_items, rel_lo=rel_lo, rel_hi=rel_hi)
    detector_obj = get_feature_detector(pth=detector_pth, device=opts.device, num_gpus=opts.num_gpus, rank=opts.rank, verbose=progress.verbose)
    flags = _label_flags(detector_pth)

    # Main loop.
    with torch.no_grad():
        for samples, _labels, real in walk:
            bbox_real = samples['bboxes'].to(opts.device).to(torch.float32)
            bbox_class = samples['labels'].to(opts.device).to(torch.int64)
            padding_mask = ~samples['mask'].to(opts.device).to(torch.bool)
            features = detector_obj.model.extract_features(bbox_real, bbox_class, padding_mask, **flags)
            stats.append_torch(_keep(features, real), num_gpus=opts.num_gpus, rank=opts.rank)
            progress.update(min(stats.num_items * opts.num_gpus, walk.num_items))
    stats.reduce(opts.num_gpus, opts.rank, per_rank_items=walk.per_rank, total_items=walk.num_items)

    # Save to cache.
    if cache_file is not None and opts.rank == 0:
        os.makedirs(os.path.dirname(cache_file), exist_ok=True)
        temp_file = cache_file + '.' + uuid.uuid4().hex
        stats.save(temp_file)
        os.replace(temp_file, cache_file) # atomic
    return stats

#----------------------------------------------------------------------------

def _generator_batches(opts, walk, dataset):
    """(batch, bbox_fake, real) per step: the batch assembled as the training loop does, G in eval mode under no_grad, gen_z drawn per batch as
    in the reference (:282)."""
    from ..training.training_loop import assemble_batch
    G = opts.G
    was_training = G.training
    G.eval()
    c_iter = iterate_random_labels(opts=opts, batch_size=walk.batch_size)
    try:
        with torch.no_grad():
            for samples, labels, real in walk:
                bt = assemble_batch(samples, labels, G, dataset.background_size_for_training, opts.device, page_filter=opts.background_filter)
                B, N = bt['bbox_class'].shape
                gen_z = torch.randn([B, N, G.z_dim], dtype=torch.float32, device=opts.device)
                bbox_fake = G(z=gen_z, bbox_class=bt['bbox_class'], bbox_real=bt['bbox_real'], bbox_text=bt['bbox_text'], bbox_patch=bt['bbox_patch'],
                              padding_mask=bt['padding_mask'], background=bt['background'], c=next(c_iter)[:B], **opts.G_kwargs)
                yield bt, bbox_fake.detach(), real
    finally:
        G.train(was_training)


def compute_feature_stats_for_generator(opts, detector_pth, detector_kwargs, rel_lo=0, rel_hi=1, batch_size=None, data_loader_kwargs=None, max_items=None, batch_gen=None, **stats_kwargs):
    dataset = _construct(opts.dataset_kwargs)
    walk = _ItemWalk(opts, dataset, max_items, batch_size, data_loader_kwargs)
    stats = FeatureStats(max_items=walk.num_items, **stats_kwargs)
    progress = opts.progress.sub(tag='generator features', num_items=walk.num_items, rel_lo=rel_lo, rel_hi=rel_hi)
    detector_obj = get_feature_detector(pth=detector_pth, device=opts.device, num_gpus=opts.num_gpus, rank=opts.rank, verbose=progress.verbose)
    flags = _label_flags(detector_pth)
    for bt, bbox_fake, real in _generator_batches(opts, walk, dataset):
        features = detector_obj.model.extract_features(bbox_fake, bt['bbox_class'], bt['padding_mask'], **flags)
        stats.append_torch(_keep(features, real), num_gpus=opts.num_gpus, rank=opts.rank)
        progress.update(min(stats.num_items * opts.num_gpus, walk.num_items))
    return stats.reduce(opts.num_gpus, opts.rank, per_rank_items=walk.per_rank, total_items=walk.num_items)

#----------------------------------------------------------------------------

def compute_maxIoU_overlap_alignment_wrapper(opts, rel_lo=0, rel_hi=1, batch_size=None, data_loader_kwargs=None, max_items=None, **stats_kwargs):
    from .metric_layoutnet import compute_alignment, compute_overlap
    dataset = _construct(opts.dataset_kwargs)
    walk = _ItemWalk(opts, dataset, max_items, batch_size, data_loader_kwargs)
    names = ('bbox_real', 'bbox_fake', 'bbox_class', 'mask', 'overlap', 'alignment')
    stats = {k: FeatureStats(max_items=walk.num_items, capture_all=True, **stats_kwargs) for k in names}
    progress = opts.progress.sub(tag='calculate maximum IoU', num_items=walk.num_items, rel_lo=rel_lo, rel_hi=rel_hi)
    for bt, bbox_fake, real in _generator_batches(opts, walk, dataset):
        mask = ~bt['padding_mask']
        vals = dict(bbox_real=bt['bbox_real'], bbox_fake=bbox_fake, bbox_class=bt['bbox_class'], mask=mask,
                    overlap=compute_overlap(bbox_fake, mask).unsqueeze(-1), alignment=compute_alignment(bbox_fake, mask).unsqueeze(-1))
        for k in names:
            stats[k].append_torch(_keep(vals[k], real), num_gpus=opts.num_gpus, rank=opts.rank)
        progress.update(min(stats['bbox_real'].num_items * opts.num_gpus, walk.num_items))
    for k in names:
        stats[k].reduce(opts.num_gpus, opts.rank, per_rank_items=walk.per_rank, total_items=walk.num_items)
    return tuple(stats[k] for k in names)

#----------------------------------------------------------------------------
