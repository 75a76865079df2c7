"""UNetDS2GN feature extractor on the HIP library: the same network as
`feature_net.UNetDS2GN` (mvsnet/cnn_wrapper/mvsnetworks.py:53-115), every layer one launch of
`mvs_conv2d_gn_f32` / `mvs_deconv2d_gn_f32` with the producer's GroupNorm (+ReLU) folded into the
consumer's load (csrc/unet2d.hip).  Same constructor and call signature as the PyTorch module, so
`MVSNetWeights` can hold either; the PyTorch/MIOpen module stays as the reference implementation of
the glue (north_star) and as the cross-check in tests.

The host side reads the layer table of `feature_net.tower_layers` (channels, sizes, who applies ReLU) and launches every
layer through `launch_layer` -- the one place under mvsnet_amd/ that calls the two entry points; the training towers
(`feature_net_train`) use the same function for their forward pass and for the input gradients of their backward pass.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .feature_net import TowerLayer, layer_sizes, tower_layers_of


# The encoder's side branches (mvsnetworks.py:66-84) depend on ONE layer of the stride-2 chain each and are only read again by the
# decoder: with `side_streams` they run on streams of their own beside the chain 1_0 .. 4_2 -> 5_0 (launch-bound low-resolution
# layers) instead of in line with it.
SIDE_BRANCH = {"2dconv0_1": 0, "2dconv0_2": 0, "2dconv1_1": 1, "2dconv1_2": 1,
               "2dconv2_1": 2, "2dconv2_2": 2, "2dconv3_1": 3, "2dconv3_2": 3}      # branch index; stream = index % side_streams


def fork_join_layers(layers):
    """Layers (or "data") whose output is read by a layer of the other kind (chain <-> side branch)."""
    return {s_ for l in layers for s_ in l.srcs if (l.name in SIDE_BRANCH) != (s_ in SIDE_BRANCH)}


class Source(NamedTuple):
    """What a layer loads: a raw (V,H,W,C) tensor and what normalises it on the load -- the producer's GroupNorm sums, gamma,
    beta and whether ReLU follows; all None / 0 for the image and for the gradients of the backward pass."""
    tensor: torch.Tensor
    stats: Optional[torch.Tensor] = None
    gamma: Optional[torch.Tensor] = None
    beta: Optional[torch.Tensor] = None
    relu: int = 0


_NO_SOURCE = Source(None)


def launch_layer(lib, l, sources, w_raw, w_prepared, V, h, w, y, stats_out, st):
    """One layer `l` over V inputs of h x w on the stream handle `st`: `sources` one Source per entry of l.srcs, `w_prepared`
    the kernel in the layout the kernel reads (transposed layers: or None, then `w_raw` in the TensorFlow layout is
    gathered), `y` the raw output, `stats_out` its GroupNorm slot sums (None: not wanted)."""
    p, a = _lib.ptr, sources[0]
    if l.kind == "dg":
        _lib.check(lib.mvs_deconv2d_gn_f32(p(a.tensor), p(a.stats), p(a.gamma), p(a.beta), l.cins[0], a.relu, p(w_raw), p(w_prepared),
                                           V, h, w, l.cout, p(y), p(stats_out), st), "mvs_deconv2d_gn_f32")
    else:
        b, c2 = (sources[1], l.cins[1]) if len(sources) > 1 else (_NO_SOURCE, 0)
        _lib.check(lib.mvs_conv2d_gn_f32(p(a.tensor), p(a.stats), p(a.gamma), p(a.beta), l.cins[0], a.relu,
                                         p(b.tensor), p(b.stats), p(b.gamma), p(b.beta), c2, b.relu,
                                         p(w_prepared), V, h, w, l.cout, l.k, l.stride, p(y), p(stats_out), st), "mvs_conv2d_gn_f32")


class LayerWeights(NamedTuple):
    prepared: Optional[torch.Tensor]                       # None: a transposed layer the library runs on the raw kernel
    raw: Optional[torch.Tensor]                            # transposed layers only
    gamma: Optional[torch.Tensor]
    beta: Optional[torch.Tensor]


class _Step(NamedTuple):
    """One layer of a pass: what launch_layer takes besides the sources and the stream."""
    layer: TowerLayer
    weights: LayerWeights
    h: int
    w: int
    y: torch.Tensor
    stats_out: Optional[torch.Tensor]


class _Pass(NamedTuple):
    """The leading V views of a set of buffers."""
    data: torch.Tensor                                     # (V,H,W,4): the image padded 3 -> 4 channels (channel 3 stays 0)
    steps: list                                            # one _Step per layer; the last one's y is the features


class _Buffers(NamedTuple):
    capacity: int                                          # views the tensors below are sized for
    acts: dict                                             # layer -> raw output (capacity, ho, wo, cout)
    stat_offsets: dict                                     # layer -> start of its slot sums in `stats`
    stats: torch.Tensor                                    # float64 slab of every layer's GroupNorm slot sums
    data: torch.Tensor
    csum: torch.Tensor                                     # workspace of mvs_center_images_u8_f32
    sizes: list                                            # feature_net.layer_sizes of the image size
    passes: dict                                           # V -> _Pass


class HipUNetDS2GN:
    """``params`` in TensorFlow variable layouts as for `UNetDS2GN` (conv (k,k,Cin,Cout), transposed
    conv (k,k,Cout,Cin), GroupNorm gamma/beta).  `side_streams`: HIP streams beside the caller's for the encoder's side
    branches (forked from / joined to the caller's stream with events inside every call): 0 = everything in line, 1 .. 4 = that
    many, "auto" (default) = decided by MEASUREMENT at the first call of an input shape: two candidate pairs of streams and the
    in-line pass are timed (three passes each, the only synchronising calls this class makes) and the fastest is kept -- which
    hardware queue a HIP stream lands on depends on what else the process created, and a side stream that shares the caller's
    compute pipe makes the pass SLOWER (measured: 1 807 against 1 055 us with one side stream on the wrong pipe, 985 with two on
    others; tools/pipe_probe.hip, round 3).  Under hipGraph capture an undecided shape runs in line."""

    takes_uint8 = True                                     # __call__ standardises decoded uint8 images itself

    def __init__(self, params, device="cuda", side_streams="auto"):
        self.device = torch.device(device)
        self.side_streams = side_streams if side_streams == "auto" else int(side_streams)
        self._streams = None
        self._choice = {}                                  # (H, W) -> list of side streams (possibly empty)
        self.table = table = tower_layers_of({name: np.asarray(p["w"]) for name, p in params.items()})
        self._fork_join = fork_join_layers(table)
        lib = _lib.load()
        self.slots = lib.mvs_gn_stat_slots()               # partial GroupNorm accumulators per (view, group)
        self.layers = [(l, self._upload(lib, l, params[l.name])) for l in table]
        torch.cuda.synchronize(self.device)
        self.out_channels = table[-1].cout
        self._bufs, self._retired = {}, []

    def _upload(self, lib, l, p):
        """One layer's variables on the device, the kernel laid out for mvs_conv2d_gn_f32 / mvs_deconv2d_gn_f32."""
        w = np.asarray(p["w"], np.float32)
        wraw = wd = None
        if l.kind == "dg":
            wraw = torch.as_tensor(w).contiguous().to(self.device)
            n = lib.mvs_deconv2d_prepared_floats(l.cins[0], l.cout)
            if n:                                          # MFMA path; otherwise the VALU gather on the raw weights
                wd = torch.empty(n, dtype=torch.float32, device=self.device)
                _lib.check(lib.mvs_deconv2d_prepare_f32(_lib.ptr(wraw), l.cins[0], l.cout, _lib.ptr(wd), _lib.stream_ptr()),
                           "mvs_deconv2d_prepare_f32")
        else:
            if l.srcs == ("data",):                        # zero weights for the padding channel
                w = np.concatenate([w, np.zeros(w.shape[:2] + (1, l.cout), np.float32)], axis=2)
            c1, c2 = l.cins[0], (l.cins[1] if len(l.cins) > 1 else 0)
            wd = torch.empty(lib.mvs_conv2d_prepared_floats(l.k, c1, c2, l.cout), dtype=torch.float32, device=self.device)
            wt = torch.as_tensor(w).contiguous().to(self.device)
            _lib.check(lib.mvs_conv2d_prepare_f32(_lib.ptr(wt), l.k, c1, c2, l.cout, _lib.ptr(wd), _lib.stream_ptr()),
                       "mvs_conv2d_prepare_f32")
        g = b = None
        if l.kind != "c":
            g = torch.as_tensor(np.asarray(p["gamma"], np.float32)).to(self.device)
            b = torch.as_tensor(np.asarray(p["beta"], np.float32)).to(self.device)
        return LayerWeights(wd, wraw, g, b)

    def _plan(self, V, H, W, slot=0):
        """Activation buffers and one float64 slab of GroupNorm sums for a (V, H, W) input (`slot`: independent sets of buffers
        for passes that run concurrently on different streams) -> the set and its _Pass for V.  One set per image size, sized
        for the largest V seen so far: a smaller batch uses the leading V views of every buffer (V is the outermost dimension
        of all of them), so a session whose groups bring 1 .. 16 new images allocates once or twice, not once per distinct V."""
        key = (H, W, slot)
        held = self._bufs.get(key)
        if held is None or held.capacity < V:
            sizes = layer_sizes(self.table, H, W)
            acts, offs, total = {}, {}, 0
            for l, (_h, _w, ho, wo) in zip(self.table, sizes):
                acts[l.name] = torch.empty((V, ho, wo, l.cout), dtype=torch.float32, device=self.device)
                offs[l.name] = total
                total += V * (l.cout // 8) * 2 * self.slots
            stats = torch.zeros(total, dtype=torch.float64, device=self.device)
            data = torch.zeros((V, H, W, 4), dtype=torch.float32, device=self.device)
            csum = torch.empty(_lib.load().mvs_center_images_workspace_bytes(V) // 8, dtype=torch.int64, device=self.device)
            if held is not None:                            # a pass on another stream may still be reading the smaller set: keep it
                self._retired.append(held)
            held = self._bufs[key] = _Buffers(V, acts, offs, stats, data, csum, sizes, {})
        if V not in held.passes:
            steps = []
            for (l, wt), (h, w, _ho, _wo) in zip(self.layers, held.sizes):
                o = held.stat_offsets[l.name]
                so = held.stats[o:o + V * (l.cout // 8) * 2 * self.slots] if l.kind != "c" else None
                steps.append(_Step(l, wt, h, w, held.acts[l.name][:V], so))
            held.passes[V] = _Pass(held.data[:V], steps)
        return held, held.passes[V]

    def _side_streams_for(self, x):
        """The side streams of this input shape (see the class docstring)."""
        key = tuple(x.shape[1:3])                          # per image size: the pipes do not depend on the batch
        if self.side_streams != "auto":
            ns = self.side_streams
            if ns and self._streams is None:
                self._streams = [torch.cuda.Stream(self.device) for _ in range(ns)]
            return self._streams[:ns] if ns else []
        if key in self._choice:
            return self._choice[key]
        if torch.cuda.is_current_stream_capturing():
            return []
        if self._streams is None:
            self._streams = [torch.cuda.Stream(self.device) for _ in range(4)]
        import time
        best, best_t = [], None
        for cand in ([], self._streams[0:2], self._streams[2:4]):
            self._run(x, cand)                             # warm: plan buffers, first launches
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            for _ in range(3):
                self._run(x, cand)
            torch.cuda.synchronize(self.device)
            t_ = time.perf_counter() - t0
            if best_t is None or t_ < 0.97 * best_t:       # a side-stream set has to win by 3 % against what is kept
                best, best_t = cand, t_
        self._choice[key] = best
        return best

    @torch.no_grad()
    def __call__(self, images):
        """images (V,H,W,3) channel-last -> features (V,H/4,W/4,C) contiguous.  float32: the centred images as the reference's
        graph takes them; uint8: the DECODED images, standardised per image and channel on the device on their way into the
        first layer's input (mvs_center_images_u8_f32 = mvs_data_generation/utils.py:33-38; a session uploads a quarter of the
        bytes and no float copy of the batch exists outside the plan's buffers)."""
        x = images.to(self.device) if images.dtype == torch.uint8 else images.to(self.device, torch.float32)
        if x.shape[1] % 16 or x.shape[2] % 16:
            raise ValueError("UNetDS2GN needs image sizes divisible by 16")
        return self._run(x, self._side_streams_for(x))

    def _run(self, x, side, slot=0):
        lib = _lib.load()
        V, H, W, _ = x.shape
        bufs, this = self._plan(V, H, W, slot)
        bufs.stats.zero_()
        if x.dtype == torch.uint8:
            x = x.contiguous()
            _lib.check(lib.mvs_center_images_u8_f32(_lib.ptr(x), V, H, W, _lib.ptr(this.data), _lib.ptr(bufs.csum), _lib.stream_ptr()),
                       "mvs_center_images_u8_f32")
        else:
            this.data[..., :3] = x
        main = torch.cuda.current_stream(self.device)
        ns = len(side)
        done = {"data": main.record_event()} if ns else {}     # layer -> event, for layers read from another stream
        src_of = {"data": Source(this.data)}
        where = {"data": main}
        for l, wt, h, w, y, so in this.steps:
            name = l.name
            st_ = side[SIDE_BRANCH[name] % ns] if ns and name in SIDE_BRANCH else main
            for s_ in l.srcs:                              # producers on another stream: wait for their event
                if where[s_] is not st_:
                    if s_ not in done:
                        done[s_] = where[s_].record_event()
                    st_.wait_event(done[s_])
            launch_layer(lib, l, [src_of[s_] for s_ in l.srcs], wt.raw, wt.prepared, V, h, w, y, so, C.c_void_p(st_.cuda_stream))
            # consumers apply this layer's GroupNorm: ReLU after conv_gn, none after deconv_gn (network.py:357)
            src_of[name] = Source(y, so, wt.gamma, wt.beta, l.relu)
            where[name] = st_
            if ns and name in self._fork_join:             # read from another stream later: its event is recorded right behind it
                done[name] = st_.record_event()
        return this.steps[-1].y.clone()
