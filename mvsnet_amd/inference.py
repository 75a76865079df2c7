"""Entry point mirroring `python -m mvsnet.inference` (mvsnet/inference.py:83-145):

    python -m mvsnet_amd.inference --input_dir <session> [--output_dir ...] --view_num 5 --max_d 192 \
        --width 640 --height 512 --regularization 3DCNN [--weights weights.npz]

One process per GPU; under torch.distributed.run the clusters (reference views) of the session are
sharded round-robin across ranks with no collective on the data path.  --model_dir /
--ckpt_step restore a TensorFlow checkpoint of the reference (mvsnet_amd/tf_checkpoint.py, no TF
needed); without them (and without --weights) the networks are randomly initialised -- no checkpoint
exists offline -- which still exercises the full pipeline and output formats.
"""
from __future__ import annotations

import argparse
import logging
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from functools import partial

import numpy as np

logger = logging.getLogger("mvsnet_amd.inference")


def build_weights(config, device, weights_path=None, model_dir=None, ckpt_step=None, extractor="hip"):
    """Weights from (in order of preference) a TensorFlow checkpoint of the reference
    (<model_dir>/<regularization>/<network_mode>/model.ckpt-<ckpt_step>, inference.py:23-27 +
    utils.py:75-96), an .npz of parameter dictionaries, or a seeded random initialisation."""
    from . import synthetic as S
    from .model import MVSNetWeights
    if model_dir:
        from . import tf_checkpoint as ck
        prefix = ck.model_path(ck.ckpt_path(model_dir, config.regularization, config.network_mode), ckpt_step)
        params = ck.load_mvsnet_params(prefix, config.network_mode, config.regularization,
                                       refinement=config.refinement_network if config.refinement else None)
        logger.info("restored %s", prefix)
        return MVSNetWeights.from_numpy(config.network_mode, unet=params["unet"], regnet=params["regnet"],
                                        gru=params["gru"], device=device, refine=params.get("refine"),
                                        refine_type=config.refinement_network, extractor=extractor)
    if weights_path:
        z = np.load(weights_path, allow_pickle=True)
        unet, regnet, gru = z["unet"].item(), z["regnet"].item(), z["gru"].item()
    else:
        unet = S.make_unet_params(config.network_mode, seed=3)
        regnet = S.make_regnet_params(config.network_mode, seed=1)
        gru = S.make_gru_params(config.network_mode, seed=2,
                                in_channels=4 * S.base_filter(config.network_mode))
    refine = None
    if config.refinement:
        from .refine import make_refine_params
        refine = make_refine_params(config.refinement_network, config.network_mode,
                                    4 + int(config.refine_with_confidence), seed=4)
    return MVSNetWeights.from_numpy(config.network_mode, unet=unet, regnet=regnet, gru=gru, device=device,
                                    refine=refine, refine_type=config.refinement_network, extractor=extractor)


def center_images_device(u8):
    """mvs_data_generation/utils.py:33-38 (per-image, per-channel standardisation) on the device: (n,H,W,3) uint8 ->
    float32 (x - mean) / (sqrt(var) + 1e-8) with the moments accumulated in float64.  PyTorch restatement of
    mvs_center_images_u8_f32 (csrc/center_images.hip, which the HIP towers call themselves when they are given uint8): used for the
    torch extractor and as the bit-for-bit cross-check in tests.  (The reference's numpy float32 reductions keep running sums
    over the leading axes: ~1e-3 relative away from the exact moments at 640 x 512; tests/test_gpu_unet.py.)"""
    import torch
    x = u8.to(torch.float32)
    # float64 ACCUMULATION of float32 terms that are exact (grey levels and their squares are integers below 2^16): the sums are
    # exact, the moments carry float64 rounding only -- without materialising a float64 copy of the batch (round 3 did: 8 bytes
    # per element through five elementwise kernels)
    n = float(x.shape[1] * x.shape[2])
    mean = x.sum(dim=(1, 2), keepdim=True, dtype=torch.float64) / n
    var = ((x * x).sum(dim=(1, 2), keepdim=True, dtype=torch.float64) / n - mean * mean).clamp_(min=0.0)
    return ((x - mean.float()) / (var.sqrt().float() + 0.00000001)).contiguous()


_DEVICE_WARM = set()


def warm_device_one_offs(device, centre):
    """Once per process and device: the torch kernels of the session's glue (a stack, a copy; with `centre` -- the torch
    extractor -- the reductions and elementwise kernels of `center_images_device`) are launched on a 16 x 16 image so that their
    code objects load -- 40-100 ms of first-use cost each on this stack -- WHILE the worker processes decode the session's
    first images, not after they have arrived (tools/r6_first_pass.py: a one-scan process's first pass)."""
    import torch
    if (device, centre) in _DEVICE_WARM:
        return
    _DEVICE_WARM.add((device, centre))
    z = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=device)
    f = center_images_device(z) if centre else z.to(torch.float32)
    torch.stack([f[0], f[1]]).clone()
    torch.cuda.Event(enable_timing=True).record()


class FeatureCache:
    """Per-image feature maps of a session, least-recently-used first out.

    `fill(group, tower)` makes every key of one group of reference views available and PINS them in `self.group` until the next
    `fill`: eviction only ever removes entries that the current group does not use, and `get` reads the pinned dict, so a key
    that was a hit when the group was formed cannot disappear before the group's last reference view has read it (round 3's FIFO
    of 256 entries evicted while it inserted: a session whose covisibility lists reach back more than `limit` images -- loop
    closures, score-ranked pair.txt -- raised KeyError outside the per-view try / except and ended the whole run)."""

    def __init__(self, limit=256):
        from collections import OrderedDict
        self.limit = max(1, int(limit))
        self.entries = OrderedDict()
        self.group = {}
        self.hits = self.misses = 0

    def fill(self, keyed_images, tower):
        """keyed_images: iterable of (key, image) over all views of the group (repeats allowed); tower(list of images) ->
        indexable batch of feature maps, called once for the images the cache misses."""
        self.group = {}
        need = {}
        for k_, img in keyed_images:
            if k_ in self.group or k_ in need:
                continue
            if k_ in self.entries:
                self.entries.move_to_end(k_)
                self.group[k_] = self.entries[k_]
                self.hits += 1
            else:
                need[k_] = img
                self.misses += 1
        if need:
            fb = tower(list(need.values()))
            for j, k_ in enumerate(need):
                self.group[k_] = self.entries[k_] = fb[j]
        while len(self.entries) > self.limit:                    # oldest first; the group's own keys are the newest
            self.entries.popitem(last=False)

    def get(self, keys):
        return [self.group[k_] for k_ in keys]


class SessionLoader:
    """Clusters of a session-format generator prepared with the per-IMAGE work on worker processes (host_pool.HostPool):
    `submit(c)` hands the cluster's images that no earlier cluster asked for to the pool and returns at once, `result(handle)`
    gives what `gen.prepare(c, center=False)` gives -- the same functions, run in the workers -- except that the image stacks
    come back as LISTS of per-view uint8 arrays (no (N,H,W,3) copy on this thread).  Image sizes (needed for the cluster's
    scale-to-cover factor before anything is decoded, mvs_cluster.py:178-192) come from the files' headers."""

    def __init__(self, gen, pool, limit=192, pin_device=None):
        from collections import OrderedDict
        self.gen, self.pool, self.limit, self.pin_device = gen, pool, limit, pin_device
        self.cams = {}                               # (session, index, depth range) -> camera: one build per image and call
        self.images = OrderedDict()                  # (session, index, rescale) -> Future of (cropped, output image, shape, seconds)
        self.sizes = {}
        self.load_seconds = 0.0
        self._counted = set()

    def _size(self, c, i):
        key = (c.session_dir, i)
        hit = self.sizes.get(key)
        if hit is None:
            from PIL import Image
            with Image.open(c.image_path(i)) as im:  # header only: nothing is decoded
                hit = self.sizes[key] = (im.size[1], im.size[0], 3)
        return hit

    def submit(self, c):
        g = self.gen
        sizes = [self._size(c, i) for i in c.indices]
        c.original_image_shape = sizes[0]
        c.rescale = max(max(float(g.image_height) / s_[0] for s_ in sizes), max(float(g.image_width) / s_[1] for s_ in sizes))
        futs = []
        for i in c.indices:
            key = (c.session_dir, i, round(float(c.rescale), 12))
            f = self.images.get(key)
            if f is None:
                f = self.images[key] = self.pool.load_image(c.image_path(i), c.rescale, g.image_width, g.image_height,
                                                            g.base_image_size, g.output_scale, pin_device=self.pin_device)
                while len(self.images) > self.limit:
                    self.images.popitem(last=False)
            else:
                self.images.move_to_end(key)
            futs.append((key, f))
        return c, sizes, futs

    def result(self, handle):
        c, sizes, futs = handle
        ins, outs = [], []
        for key, f in futs:
            cr, oi, _shape, sec = f.result()
            if key not in self._counted:             # worker seconds, once per decoded image
                self._counted.add(key)
                self.load_seconds += sec
            ins.append(cr); outs.append(oi)
        cams = []
        for i in c.indices:                          # a camera is listed by ~view_num clusters: built once (round 5: 5x, on this thread)
            ck = (c.session_dir, i, c.min_depth, c.max_depth, c.depth_num, c.interval_scale)
            cam = self.cams.get(ck)
            if cam is None:
                cam = self.cams[ck] = c.load_camera(i)
            cams.append(cam)
        full_cams, out_cams = self.gen.cluster_cameras(c, cams, sizes)
        return outs, ins, out_cams, full_cams, c.ref_index


# Pinned host buffers are expensive to create (~1.5 ms each) and cheap to keep: the staging buffers of the uploads and the result
# buffers of the downloads live for the process, not for one compute_depth_maps call (a session is one call).
_PINNED_STAGING = {}                                  # (shape, dtype) -> _Staging
_PINNED_RESULTS = {}                                  # shape -> free pinned (depth, prob) buffer pairs


class _Staging:                                       # two alternating pinned upload buffers and their last copies' events
    def __init__(self):
        self.bufs, self.events, self.next = [None, None], [None, None], 0


def _upload(arrays, device):
    """Same-shape host arrays -> one device tensor of their dtype, by an asynchronous copy on the current stream: from the
    arrays' own pinned memory (host_pool.PinnedArray, no copy on this thread) or through the staging pair of their shape."""
    import torch
    arrays = list(arrays)
    n, shp, dt = len(arrays), arrays[0].shape, arrays[0].dtype
    pins = [getattr(a_, "pinned", None) for a_ in arrays]
    if all(p_ is not None for p_ in pins):
        dst = torch.empty((n,) + tuple(shp), dtype=pins[0].dtype, device=device)
        for j, p_ in enumerate(pins):
            dst[j].copy_(p_, non_blocking=True)
        return dst
    st = _PINNED_STAGING.setdefault((shp, dt), _Staging())
    i, st.next = st.next, st.next ^ 1
    if st.bufs[i] is None or st.bufs[i].shape[0] < n:
        st.bufs[i] = torch.empty((max(n, 16),) + shp, dtype=torch.from_numpy(np.empty(0, dt)).dtype).pin_memory()
    elif st.events[i] is not None:
        st.events[i].synchronize()
    view = st.bufs[i].numpy()
    for j, a_ in enumerate(arrays):
        view[j] = a_
    t_ = st.bufs[i][:n].to(device, non_blocking=True)
    st.events[i] = torch.cuda.current_stream(device).record_event()
    return t_


def _images_to_device(imgs, device, keep_uint8):
    """Images -> device: uint8 ones stay uint8 with `keep_uint8` (the HIP towers standardise them in the library) and are
    standardised here otherwise; float ones become float32."""
    import torch
    t_ = _upload(imgs, device)
    if t_.dtype == torch.uint8:
        return t_ if keep_uint8 else center_images_device(t_)
    return t_.to(torch.float32)


def _feature_keys(c, in_images, view_num):
    """Feature-cache key of each view of a cluster: an image's features only depend on the image and the (rescale, crop) it got."""
    ids = getattr(c, "indices", None) or list(getattr(c, "paths", [])[0::2])
    return [(c.session_dir, ids[v], round(float(c.rescale), 9), in_images[v].shape) if v < len(ids) else ("view", id(c), v)
            for v in range(view_num)]


class _StageClock:
    """Host seconds per stage (`tm`: this thread, the loader threads and the writer threads add to it) and GPU time between
    (start, end) event pairs of tower passes, hot paths and hot-path end -> results in pinned memory.  All event work is
    skipped without `timings`."""

    def __init__(self, timings, pool, t_wall):
        self.timings, self.on, self.pool, self.t_wall = timings, timings is not None, pool, t_wall
        # submit_*: host_gpu_submit's parts: image upload + tower launches, feature stack, hot-path launches, result hand-over
        self.tm = dict.fromkeys(("load", "wait_load", "host_gpu_submit", "write", "submit_towers", "submit_features",
                                 "submit_depth", "submit_finish"), 0.0)
        self.lock = threading.Lock()
        self.spans = {"towers": [], "hot_path": [], "d2h": []}
        self.cpu0 = None
        if self.on:
            try:
                import psutil
                self.cpu0 = (sum(psutil.Process().cpu_times()[:2]), pool.cpu_seconds() if pool is not None else 0.0)
            except Exception:                         # noqa: BLE001
                pass

    def add(self, name, seconds):
        with self.lock:
            self.tm[name] += seconds

    def timed(self, name, fn, *a):
        t0 = time.perf_counter()
        try:
            return fn(*a)
        finally:
            self.add(name, time.perf_counter() - t0)

    def mark(self):
        import torch
        return torch.cuda.current_stream().record_event(torch.cuda.Event(enable_timing=True)) if self.on else None

    def span(self, kind, start, end):
        if self.on:
            self.spans[kind].append((start, end))

    def report(self, done, n_loaders, n_writers):
        if not self.on:
            return
        import torch
        t = self.timings
        torch.cuda.synchronize()
        t.update(self.tm)
        t["wall"] = time.perf_counter() - self.t_wall
        t["depth_maps"] = done
        t["loader_threads"], t["writer_threads"] = n_loaders, n_writers
        t["host_workers"] = self.pool.workers if self.pool is not None else 0
        if self.cpu0 is not None:
            import psutil
            t["host_cpu"] = (sum(psutil.Process().cpu_times()[:2]) - self.cpu0[0]) + \
                            ((self.pool.cpu_seconds() or 0.0) - (self.cpu0[1] or 0.0) if self.pool is not None else 0.0)
        for kind, spans in self.spans.items():
            t[kind] = sum((a_.elapsed_time(b_) * 1e-3 for a_, b_ in spans), 0.0)


class _ResultSink:
    """`put`: a view's (depth, prob) -> a pinned host pair by an asynchronous copy on the compute stream, so this thread never
    waits for the GPU (round 2 called .cpu() here) -> a writer thread, which waits for the copy's event and writes the files or
    hands them to the worker processes.  At most 8 pairs are in flight: `put` blocks for a free one."""

    WRITERS = 4

    def __init__(self, config, output_dir, pool, clock):
        self.config, self.output_dir, self.pool, self.clock = config, output_dir, pool, clock
        self.slots = threading.BoundedSemaphore(8)
        self.lock = threading.Lock()
        self.writer = ThreadPoolExecutor(max_workers=self.WRITERS)
        self.writes, self.pool_writes = [], []

    def put(self, d, p, out_images, in_images, out_cams, full_cams, index):
        """Returns the event of the copy to pinned memory."""
        import torch
        self.slots.acquire()
        with self.lock:
            free = _PINNED_RESULTS.setdefault(tuple(d.shape), [])
            pair = free.pop() if free else None
        if pair is None:
            pair = (torch.empty(d.shape, dtype=torch.float32).pin_memory(), torch.empty(p.shape, dtype=torch.float32).pin_memory())
        pair[0].copy_(d, non_blocking=True)
        pair[1].copy_(p, non_blocking=True)
        copied = torch.cuda.current_stream().record_event(torch.cuda.Event(enable_timing=self.clock.on))
        self.writes.append(self.writer.submit(self._write, pair, copied, out_images, in_images, out_cams, full_cams, index))
        return copied

    def _write(self, pair, copied, out_images, in_images, out_cams, full_cams, index):
        from . import predictlib as pl
        cfg = self.config
        try:                                          # the pair and its slot are released exactly once, on every path
            copied.synchronize()
            if cfg.refinement and cfg.upsample_before_refinement:         # full-size outputs (predictlib.py:107-115)
                from .mvs_data_generation import center_image           # the reference writes the STANDARDISED input image here
                img0 = center_image(in_images[0]) if in_images[0].dtype == np.uint8 else in_images[0]
                args = (img0, full_cams[0], index, cfg.visualize, 1.0 / cfg.sample_scale)
            else:
                args = (out_images[0], out_cams[0], index, cfg.visualize, None)
            if self.pool is None:
                return self.clock.timed("write", pl.write_output_slice, self.output_dir, pair[0].numpy(), pair[1].numpy(), *args)
            # private copies (the executor pickles them later, on its feeder thread), then the pinned pair is free again
            dn, pn = np.array(pair[0].numpy()), np.array(pair[1].numpy())
        finally:
            with self.lock:
                _PINNED_RESULTS[tuple(pair[0].shape)].append(pair)
            self.slots.release()
        f_ = self.pool.write_outputs(self.output_dir, dn, pn, np.asarray(args[0]), np.asarray(args[1]), *args[2:])
        with self.lock:
            self.pool_writes.append(f_)

    def close(self):
        """Waits for every write (raising what a writer raised) and returns the worker processes' write seconds."""
        for w_ in self.writes:
            w_.result()
        seconds = sum((f_.result() for f_ in self.pool_writes), 0.0)
        self.writer.shutdown()
        return seconds


class _ClusterFeed:
    """Loads clusters `ahead` of the one in hand -- session format on the worker processes (SessionLoader) or on loader threads
    as uint8, upstream pair.txt on loader threads standardised on the host -- and yields them in groups of up to `chunk`,
    skipping and logging those that fail."""

    def __init__(self, clusters, gen, pool, device, clock, n_loaders, ahead=16):
        self.gen, self.clock = gen, clock
        self.session_loader = SessionLoader(gen, pool, pin_device=device.index) if pool is not None else None
        self.loader = ThreadPoolExecutor(max_workers=n_loaders)
        self.it, self.pending = iter(clusters), []
        for _ in range(ahead):
            self._submit_next()

    def _submit_next(self):
        from .mvs_data_generation import Cluster
        for c in self.it:
            if type(c) is not Cluster:
                load = self.loader.submit(self.clock.timed, "load", self.gen.prepare, c).result
            elif self.session_loader is None:
                load = self.loader.submit(self.clock.timed, "load", self.gen.prepare, c, False).result
            else:
                try:
                    load = partial(self.session_loader.result, self.session_loader.submit(c))
                except Exception as e:                # an unreadable header: skip-and-log like a failed load
                    logger.warning("skipping cluster %s/%d: %s", c.session_dir, c.ref_index, e)
                    continue
            self.pending.append((c, load))
            return

    def groups(self, chunk):
        while self.pending:
            group, t0 = [], time.perf_counter()
            while self.pending and len(group) < chunk:
                c, load = self.pending.pop(0)
                self._submit_next()
                try:
                    group.append((c, load()))
                except Exception as e:                # skip-and-log per reference view
                    logger.warning("skipping cluster %s/%d: %s", c.session_dir, c.ref_index, e)
            self.clock.add("wait_load", time.perf_counter() - t0)
            if group:
                yield group

    def close(self):
        """Returns the worker processes' load seconds (the loader threads' are in the clock already)."""
        self.loader.shutdown()
        return self.session_loader.load_seconds if self.session_loader is not None else 0.0


def _starts_new_sweep(batch, shape, depth_num):
    """A recurrent sweep takes views of one feature shape and depth count: a view unlike the pending ones sends them off first."""
    return bool(batch) and (batch[0][0].shape != shape or batch[0][2] != depth_num)


class _GruBatcher:
    """Up to `views` reference views of the GRU regulariser in one sweep (mvs_gru_wta_batch_f32), a DepthPlan per shape."""

    def __init__(self, config, weights, device, views, sink, clock):
        self.config, self.weights, self.device, self.views, self.sink, self.clock = config, weights, device, views, sink, clock
        self.batch, self.plans = [], {}

    def add(self, features, cams, depth_num, depth_start, depth_end, rest):
        if _starts_new_sweep(self.batch, features.shape, depth_num):
            self.flush()
        self.batch.append((features, cams, depth_num, depth_start, depth_end, rest))
        if len(self.batch) >= self.views:
            self.flush()

    def flush(self):
        if not self.batch:
            return
        from .model import DepthPlan, wta_depth_values
        cfg = self.config
        _, Hf, Wf, Cf = self.batch[0][0].shape
        key = (self.batch[0][2], Hf, Wf, Cf)
        plan = self.plans.get(key)
        if plan is None:
            plan = self.plans[key] = DepthPlan(cfg.view_num, key[0], Hf, Wf, Cf, self.weights, "GRU", self.device, views=self.views)
        dvs = []
        for v, (_f, cams, D, start, end, _rest) in enumerate(self.batch):
            interval = float((np.float32(end) - np.float32(start)) / (np.float32(D) - np.float32(1)))      # model.py:606-607
            plan.set_cameras(cams, start, interval, end, cfg.inverse_depth, view=v)
            dvs.append(wta_depth_values(D, start, end, cfg.inverse_depth))
        m0 = self.clock.mark()
        dd, pp_ = plan.run_gru_batch([b_[0] for b_ in self.batch], dvs)
        m1 = self.clock.mark()
        self.clock.span("hot_path", m0, m1)
        for v, b_ in enumerate(self.batch):
            # copied out in stream order, before the next sweep overwrites the plan's buffers
            copied = self.sink.put(dd[v], pp_[v], *b_[5])
            if v == 0:
                self.clock.span("d2h", m1, copied)
        self.batch = []


def compute_depth_maps(input_dir, config=None, weights=None, device=None, timings=None, gru_views=4,
                       feature_cache_limit=256, host_workers=None, **kwargs):
    """mvsnet/inference.py:83-119.  Returns the number of depth maps this rank wrote.

    `timings` (a dict) receives the stage breakdown of the run in seconds: wall, load (decode + resize + crop + centre on the
    loader threads, summed over threads), wait_load (this thread blocked on the loaders), towers / hot_path / d2h (GPU time from
    stream events, host -> device copies of the images included in towers), host_gpu_submit (this thread enqueueing), write (file
    writers, summed over threads).  `gru_views`: reference views per recurrent sweep (mvs_gru_wta_batch_f32) with the GRU
    regulariser.  `host_workers`: worker PROCESSES for image decoding / rescaling and output encoding (host_pool; None = by
    core count, 0 = round 3's loader / writer threads inside this process); `timings` then also receives host_cpu = CPU
    seconds of this process and its workers."""
    import torch
    from . import host_pool, predictlib as pl, shard as sh
    from .mvs_data_generation import Cluster, make_generator

    config = config or pl.InferenceConfig()
    for k, v in kwargs.items():                       # predictlib.init_inference: kwargs -> flags
        if not hasattr(config, k):
            raise AttributeError("unknown flag %s" % k)
        setattr(config, k, v)
    rank, local_rank, world = sh.rank_world()
    if device is None:
        device = sh.bind_device(local_rank)           # one process drives one GPU
    else:
        device = torch.device(device)                 # 'cuda' without an index = the current device
        idx = device.index if device.index is not None else torch.cuda.current_device()
        torch.cuda.set_device(idx)                    # library launches go to the current device
        device = torch.device("cuda", idx)
    output_dir = pl.setup_output_dir(input_dir, config.output_dir)
    gen = make_generator(input_dir, config.view_num, config.width, config.height, config.max_d,
                           config.interval_scale, config.base_image_size, mode="inference",
                           output_scale=config.sample_scale,
                           max_clusters_per_session=config.max_clusters_per_session)
    clusters = sorted(gen.clusters, key=lambda c: (c.session_dir, c.ref_index))
    mine = sh.shard(clusters, rank, world)
    if weights is None:
        weights = build_weights(config, device)
    t_wall = time.perf_counter()
    # Like the reference's tf.data prefetch (predictlib.py:48-51), loads and writes run off this thread, which only drives the
    # GPU; since round 4 their per-image work runs in worker PROCESSES (on threads, this thread mostly waited for the GIL).
    # Loader / writer threads are the thin ends of that pipe, and the whole pipe for pair.txt projects and host_workers = 0.
    pool = host_pool.get_pool(host_workers) if any(type(c_) is Cluster for c_ in mine) else None
    clock = _StageClock(timings, pool, t_wall)
    sink = _ResultSink(config, output_dir, pool, clock)
    n_loaders = max(2, min(8, (os.cpu_count() or 4) // 2))
    feed = _ClusterFeed(mine, gen, pool, device, clock, n_loaders)
    gru = (_GruBatcher(config, weights, device, gru_views, sink, clock)
           if config.regularization == "GRU" and gru_views > 1 and not config.refinement else None)
    # the reference re-runs the towers on every source image of every cluster (model.py:392-406): SURVEY 8a R11 / 8f f2
    feature_cache = FeatureCache(feature_cache_limit)
    takes_u8 = bool(getattr(weights.unet, "takes_uint8", False))    # HipUNetDS2GN standardises uint8 input in the library
    warm_device_one_offs(device, centre=not takes_u8)
    # Uploads + towers of a group run on a stream of their own, beside the hot path of the previous group.  Their feature maps
    # are read on the compute stream: record_stream keeps the allocator from reusing a freed map that is still being read.
    t_stream, compute = torch.cuda.Stream(device), torch.cuda.current_stream(device)
    done = 0
    # 8 reference views per tower pass, their new images in one batch (~31 launches on a ~25 us floor: one image costs nearly
    # as much as sixteen).  Round 6: a ramp of 2, 4, 8 views for the first groups gained nothing (555-570 vs 567-583 maps/s).
    for group in feed.groups(chunk=8):
        t1 = time.perf_counter()
        with torch.cuda.stream(t_stream):
            m_start = clock.mark()
            feature_cache.fill(((k_, res_[1][v]) for c_, res_ in group
                                for v, k_ in enumerate(_feature_keys(c_, res_[1], config.view_num))),
                               lambda imgs: weights.unet(_images_to_device(imgs, device, keep_uint8=takes_u8)))
            clock.span("towers", m_start, clock.mark())
            towers_done = t_stream.record_event()
        compute.wait_event(towers_done)
        clock.add("submit_towers", time.perf_counter() - t1)
        # the group's cameras in ONE upload through pinned staging (a pageable .to(device) per reference view is a blocking
        # copy queued behind the previous view's kernels: it cost this thread ~0.6 ms per view)
        cams_group = _upload([np.asarray(res_[2], dtype=np.float32) for _c, res_ in group], device)
        for gi, (c, rest) in enumerate(group):
            out_images, in_images, out_cams, full_cams, index = rest
            start, t_a = time.time(), time.perf_counter()
            maps = feature_cache.get(_feature_keys(c, in_images, config.view_num))
            for m_ in maps:
                m_.record_stream(compute)
            features = torch.stack(maps).contiguous()
            clock.add("submit_features", time.perf_counter() - t_a)
            depth_start, depth_interval = float(out_cams[0, 1, 3, 0]), float(out_cams[0, 1, 3, 1])  # predictlib.set_shapes :190-197
            depth_num, depth_end = int(out_cams[0, 1, 3, 2]), float(out_cams[0, 1, 3, 3])
            if gru is not None:
                gru.add(features, cams_group[gi], depth_num, depth_start, depth_end, rest)
            else:
                # the refinement's guide is the STANDARDISED reference image (predictlib.py:86-88): only tower input may stay uint8
                ref_image = _images_to_device(in_images[0:1], device, keep_uint8=False) if config.refinement else None
                m_a, t_b = clock.mark(), time.perf_counter()
                d, p, _ = pl.get_depth_and_prob_map(None, cams_group[gi][None], depth_start, depth_interval, config, weights,
                                                    depth_num=depth_num, depth_end=depth_end, features=features,
                                                    ref_image=ref_image)
                m_depth, t_c = clock.mark(), time.perf_counter()
                clock.add("submit_depth", t_c - t_b)
                clock.span("hot_path", m_a, m_depth)
                clock.span("d2h", m_depth, sink.put(d, p, *rest))
                clock.add("submit_finish", time.perf_counter() - t_c)
            done += 1
            logger.info("Depth inference %d/%d finished. (%.3f sec/step)", done, len(mine), time.time() - start)
        clock.add("host_gpu_submit", time.perf_counter() - t1)
    if gru is not None:
        gru.flush()
    clock.add("write", sink.close())                  # surfaces write errors; all files are on disk on return
    clock.add("load", feed.close())
    clock.report(done, n_loaders, _ResultSink.WRITERS)
    return done


def main(argv=None):
    from . import ensure_miopen_workaround
    ensure_miopen_workaround("mvsnet_amd.inference")      # the torch extractor / refinement towers run ATen convolutions
    from . import predictlib as pl
    from . import shard as sh
    ap = argparse.ArgumentParser(description=__doc__)
    cfg = pl.InferenceConfig()
    for name, default in vars(cfg).items():
        if isinstance(default, bool):
            ap.add_argument("--" + name, type=lambda s: s.lower() in ("1", "true", "yes"), default=default)
        else:
            ap.add_argument("--" + name, type=type(default) if default is not None else str, default=default)
    ap.add_argument("--weights", default=None, help=".npz with 'unet', 'regnet', 'gru' parameter dicts")
    ap.add_argument("--model_dir", default=None, help="reference checkpoint root (TensorFlow V2 checkpoint, read without TF)")
    ap.add_argument("--ckpt_step", type=int, default=400000)
    ap.add_argument("--extractor", choices=("hip", "torch"), default="hip",
                    help="2D feature towers: HIP library kernels (default) or the PyTorch/MIOpen module")
    ap.add_argument("--gru_views", type=int, default=4, help="reference views per recurrent sweep (GRU regulariser)")
    ap.add_argument("--gpus", type=int, default=1,
                    help="N > 1 without a torch.distributed.run environment: start N one-GPU ranks of this command "
                         "(reference views sharded round-robin, no data-path collective)")
    ap.add_argument("--procs_per_gpu", type=int, default=1,
                    help="worker processes sharing each GPU (ranks = gpus x procs_per_gpu, collectives over gloo): the loop "
                         "load -> towers -> hot path -> write is bound by ONE Python thread per process (DESIGN section 5, "
                         "`session`), several processes per GPU fill it")
    ap.add_argument("--host_workers", type=int, default=-1,
                    help="worker processes for image decoding / rescaling and output encoding (mvsnet_amd/host_pool.py); "
                         "-1 = by core count, 0 = loader / writer threads inside this process")
    ap.add_argument("--passes", type=int, default=1,
                    help="run the whole input this many times and report all passes after the first together (throughput "
                         "measurements: the first pass pays plans, code objects and pinned buffers)")
    args = ap.parse_args(argv)
    if not (1 <= args.gru_views <= 8):                         # MVS_GRU_MAX_VIEWS of the library (mvs_gru_wta_batch_f32)
        ap.error("--gru_views must be 1..8 (reference views per recurrent sweep)")
    logging.basicConfig(level=os.environ.get("LOG_LEVEL", "INFO"))
    if args.procs_per_gpu > 1 and args.regularization == "GRU":
        # measured (round 3, 160x128, D = 192): 165 depth maps/s with one process, 53 with three -- the recurrent sweep is a
        # four-queue wavefront, and the queues of several processes share the GPU's four compute pipes
        logger.warning("--procs_per_gpu %d with the GRU regulariser: the sweeps of different processes share the GPU's compute "
                       "pipes and slow each other down; use --gru_views to put several reference views into one sweep instead",
                       args.procs_per_gpu)
    n_ranks = max(1, args.gpus) * max(1, args.procs_per_gpu)
    if n_ranks > 1 and "WORLD_SIZE" not in os.environ:         # before anything touches the GPU: the parent stays GPU-less
        import sys
        if args.procs_per_gpu > 1:                             # ranks share GPUs: RCCL wants one GPU per rank
            os.environ["MVS_DIST_BACKEND"] = "gloo"
        raise SystemExit(sh.launch_ranks(list(sys.argv[1:] if argv is None else argv), n_ranks, module="mvsnet_amd.inference",
                                         gpus=max(1, args.gpus)))
    weights_path = args.weights
    for name in vars(cfg):
        setattr(cfg, name, getattr(args, name))
    if cfg.input_dir is None:
        ap.error("--input_dir is required")
    dist = sh.init_process_group()
    # a single session, or a folder of sessions (inference.py:121-141)
    if os.path.isfile(os.path.join(cfg.input_dir, "covisibility.json")) or \
            os.path.isfile(os.path.join(cfg.input_dir, "pair.txt")):
        dirs = [cfg.input_dir]
    else:
        dirs = [os.path.join(cfg.input_dir, f) for f in sorted(os.listdir(cfg.input_dir))
                if not f.startswith(".") and not f.endswith(".txt")]
    import torch
    rank, local_rank, world = sh.rank_world()
    device = sh.bind_device(local_rank)
    weights = build_weights(cfg, device, weights_path, args.model_dir, args.ckpt_step, args.extractor)
    total, wall, t0 = 0, 0.0, time.perf_counter()
    for p_ in range(max(1, args.passes)):
        if p_ <= 1:                                   # the timed region = every pass after the first (or the only one)
            if dist is not None:
                dist.barrier()                        # the ranks start together: the rate is all maps / the slowest rank
            t0, total = time.perf_counter(), 0
        for d in dirs:
            total += compute_depth_maps(d, cfg, weights, device, gru_views=args.gru_views,
                                        host_workers=None if args.host_workers < 0 else args.host_workers)
        wall = time.perf_counter() - t0
    counts = sh.gather_counts(dist, total, device=device if dist is not None else "cpu")
    walls = sh.gather_counts(dist, wall, device=device if dist is not None else "cpu")
    devs = sh.gather_counts(dist, device.index, device=device if dist is not None else "cpu")      # the GPU each rank was bound to
    if rank == 0:
        import json
        logger.info("all dense finished: %d depth maps (%s per rank)", int(sum(counts)), counts)
        print(json.dumps({"depth_maps": int(sum(counts)), "ranks": len(counts), "procs_per_gpu": args.procs_per_gpu,
                          "devices": [int(x) for x in devs],
                          "seconds_slowest_rank": max(walls), "depth_maps_per_s": sum(counts) / max(max(walls), 1e-9),
                          "sec_per_step": max(walls) / max(sum(counts), 1), "passes": max(1, args.passes)}), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
