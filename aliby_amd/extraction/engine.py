"""
Device-side feature engine: thin Python host over the C ABI (include/aliby_hip.h).

torch is used for device buffers and the stream only; every computation is a
HIP kernel in libaliby_hip.so reached through ctypes.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from aliby_amd import _lib
from aliby_amd.extraction import features as feat


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t) -> int:
    if t is None:
        return 0
    if isinstance(t, torch.Tensor):
        return t.data_ptr()
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    raise TypeError(type(t))


def to_device_u16(a) -> torch.Tensor:
    """Host or device array -> contiguous uint16 tensor on the current GPU."""
    if isinstance(a, torch.Tensor):
        t = a
        if t.dtype == torch.int16:
            t = t.view(torch.uint16)
        if t.dtype != torch.uint16:
            raise TypeError(f"expected uint16 labels, got {t.dtype}")
        return t.cuda().contiguous()
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint16:
        if a.size and (a.min() < 0 or a.max() >= 65535):
            raise OverflowError(f"labels outside uint16 range: max={a.max()}")
        a = a.astype(np.uint16)
    return torch.from_numpy(a).cuda()


def to_device_planes(a) -> tuple[torch.Tensor, int]:
    """Pixels -> (tensor, dtype code).  <=16-bit unsigned ints are stored as uint16 (uint8 / bool with the code U8W, so that the
    texture kernel takes their grey level as skimage.util.img_as_ubyte does: unchanged); everything else is f32."""
    if isinstance(a, torch.Tensor):
        if a.dtype == torch.uint16:
            return a.cuda().contiguous(), _lib.U16
        if a.dtype == torch.uint8:
            return a.cuda().to(torch.int32).to(torch.uint16).contiguous(), _lib.U8W
        return a.cuda().to(torch.float32).contiguous(), _lib.F32
    a = np.asarray(a)
    if a.dtype in (np.uint16, np.uint8, np.bool_):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16)).cuda(), _lib.U16 if a.dtype == np.uint16 else _lib.U8W
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda(), _lib.F32


def _kdt(dtype: int) -> int:
    """dtype code as the kernels other than texture take it (U8W planes are uint16 storage)."""
    return _lib.U16 if dtype == _lib.U8W else dtype


@dataclass
class ObjectTable:
    """Compact (tile, label) table — stands in for transform_2d_to_3d's (N,Y,X) bool stack."""

    dev: torch.Tensor          # uint8 [n_obj * 32] holding aliby_object rows
    host: np.ndarray           # structured array, dtype _lib.OBJECT_DTYPE
    offsets: np.ndarray        # int32 [F+1]
    n_obj: int
    max_area: int
    max_h: int
    max_w: int
    # what the engine computes once per table (mec, _offsets_dev, radial_geometry: key -> code map, rank_planes: key -> entry);
    # None = nothing yet, which is also what an instance reads after its attribute was removed
    _mec: torch.Tensor | None = field(default=None, repr=False, compare=False)
    _offsets_dev: torch.Tensor | None = field(default=None, repr=False, compare=False)
    _binmaps: dict | None = field(default=None, repr=False, compare=False)
    _ranks: dict | None = field(default=None, repr=False, compare=False)

    @property
    def lds_resident(self) -> bool:
        """Every object window fits the LDS forms of the box- and area-sized kernels: only then may per-object launches of one context
        run side by side on several streams (the scratch rule, and what this does not guarantee: aliby_amd/csrc/object_launch.h)."""
        return self.n_obj > 0 and self.max_h * self.max_w <= 4096


class _NoTimer:
    active = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_TIMER = _NoTimer()


class _Download:
    def __init__(self, event, views):
        self.event, self.views = event, views

    def wait(self, spin: bool = True):
        if spin:
            while not self.event.query():  # polled (see aliby_wait_stream): no late wake-up
                pass
        else:
            self.event.synchronize()  # blocking, GIL released: for writer threads, where a late wake-up costs nothing
        return [v.numpy() for v in self.views]


class _Timer:
    __slots__ = ("eng", "name", "a")
    active = True

    def __init__(self, eng, name):
        self.eng, self.name = eng, name

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.a.record()
        return self

    def __exit__(self, *exc):
        b = torch.cuda.Event(enable_timing=True)
        b.record()
        self.eng._profile().setdefault(self.name, []).append((self.a, b))
        return False


class FeatureEngine:
    shared_profile = None  # set to {} to time the kernel groups of EVERY engine of the process (steps build their own engines)

    def _profile(self):
        return self.profile if self.profile is not None else FeatureEngine.shared_profile

    @property
    def ctx(self):
        """The context of the thread that is calling (aliby_amd/_lib.py default_context): an engine built on one thread and
        used on another — the runner's tilers are — never shares a scratch block with a call in flight elsewhere."""
        return _lib.default_context(self.device)

    def __init__(self, device: int | None = None):
        if not torch.cuda.is_available():
            raise _lib.AlibyHipError("no GPU visible: the HIP feature engine has no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = device
        self.lib = self.ctx.lib
        self.profile = None  # set to {} to time kernel groups with HIP events on the launch stream
        self.profile_sample = {}  # group name -> n: bracket only every n-th launch of that group
        self._sample_count = {}
        self.propagate_stats = None  # (rounds that changed a key, flag reads) of the last propagate_labels call

    # ---------------------------------------------------------------- the launch path
    def _launch(self, group, entry: str, *args) -> None:
        """Calls the C entry `entry`(context, *args, stream) of the calling thread's context on torch's current stream and raises
        what its status code stands for; bracketed as profile group `group` unless that is None."""
        with _NO_TIMER if group is None else self.timed(group):
            _lib.check(getattr(self.lib, entry)(self.ctx.handle, *args, _stream_ptr()))

    def call(self, entry: str, *args, group=None) -> None:
        """`_launch` for the package's other modules (segment/, tile/): they reach the library through an engine, not on their own."""
        self._launch(group, entry, *args)

    # ---------------------------------------------------------------- host transfer
    def to_host(self, t: torch.Tensor, copy: bool = True) -> np.ndarray:
        """Device tensor -> NumPy through a reused pinned staging buffer (pageable copies run at ~12 GB/s,
        pinned ones at PCIe rate).  copy=True returns an array that owns its memory; copy=False returns a
        view of the staging buffer, valid until the next call with the same dtype and shape."""
        if t.numel() == 0:
            return np.empty(tuple(t.shape), dtype=torch.empty(0, dtype=t.dtype).numpy().dtype)
        pool = self.__dict__.setdefault("_pinned", {})
        key = (t.dtype, tuple(t.shape)) if not copy else t.dtype
        need = t.numel()
        buf = pool.get(key)
        if buf is None or buf.numel() < need:
            buf = torch.empty(int(need * 1.25) + 1024, dtype=t.dtype, pin_memory=True)
            pool[key] = buf
        view = buf[:need].view(t.shape)
        view.copy_(t.contiguous(), non_blocking=True)
        self._launch(None, "aliby_stream_sync")  # polls an event: no late wake-up
        return view.numpy().copy() if copy else view.numpy()

    def to_host_async(self, tensors, slot: int = 0, alloc=None):
        """Start the download of `tensors` into pinned buffers on a side stream (after everything queued so far on the
        current stream) and return a handle; handle.wait() -> list of NumPy views.  The copy overlaps whatever the
        caller queues next; `slot` selects one of the reusable buffer sets (alternate it between consecutive calls)."""
        side = self.__dict__.setdefault("_copy_stream", None) or torch.cuda.Stream()
        self._copy_stream = side
        pool = self.__dict__.setdefault("_pinned_async", {})
        done = torch.cuda.Event()
        ready = torch.cuda.Event()
        ready.record()
        side.wait_event(ready)
        views = []
        with torch.cuda.stream(side):
            for i, t in enumerate(tensors):
                key = (slot, i, t.dtype)
                buf = pool.get(key) if slot is not None else None
                if alloc is not None:  # the caller's page-locked arena (aliby_amd/runner.py: reused from batch to batch)
                    buf = alloc((max(t.numel(), 1),), t.dtype)
                elif slot is None:  # a buffer of its own (readers on other threads keep it alive; torch recycles pinned blocks)
                    buf = torch.empty(max(t.numel(), 1), dtype=t.dtype, pin_memory=True)
                elif buf is None or buf.numel() < t.numel():
                    buf = pool[key] = torch.empty(int(t.numel() * 1.25) + 1024, dtype=t.dtype, pin_memory=True)
                v = buf[: t.numel()].view(t.shape)
                v.copy_(t, non_blocking=True)
                t.record_stream(side)
                views.append(v)
            done.record(side)
        return _Download(done, views)

    # ---------------------------------------------------------------- profiling
    def timed(self, name: str):
        """Context manager: brackets the enclosed launches with events on torch's current stream (the stream every
        kernel is launched on) when profiling is enabled.  Groups listed in `profile_sample` (name -> n) are
        launched hundreds of times per step: only every n-th launch is bracketed (two event records per launch
        would otherwise perturb what they measure); `collect_profile` scales the sampled average to all launches."""
        if self._profile() is None:
            return _NO_TIMER
        every = self.profile_sample.get(name, 1)
        if every > 1:
            k = self._sample_count.get(name, 0)
            self._sample_count[name] = k + 1
            if k % every:
                return _NO_TIMER
        return _Timer(self, name)

    def collect_profile(self) -> dict:
        torch.cuda.synchronize()
        out = {}
        for name, evs in (self._profile() or {}).items():
            timed_ms = float(sum(a.elapsed_time(b) for a, b in evs))
            launches = self._sample_count.get(name, len(evs)) if self.profile_sample.get(name, 1) > 1 else len(evs)
            out[name] = {"ms_total": timed_ms * launches / max(len(evs), 1), "launches": launches, "timed_launches": len(evs)}
        self._sample_count = {}
        return out

    # ------------------------------------------------------------------ z-reduction
    _REDUCED = {_lib.U16: torch.uint16, _lib.F32: torch.float32, _lib.U64: torch.uint64, _lib.F64: torch.float64}

    def reduce_z(self, t: torch.Tensor, op: int, in_dtype: int, out_dtype: int) -> torch.Tensor:
        """[..., Z, Y, X] -> [..., Y, X]: the reduction `op` (_lib.RED_MAX / RED_ADD / RED_DIV) over Z of contiguous uint16 or
        float32 planes (`in_dtype`), written as `out_dtype` (U16, F32, or NumPy's own U64 / F64; aliby_reduce_z)."""
        *lead, Z, Y, X = t.shape
        out = torch.empty((*lead, Y, X), dtype=self._REDUCED[out_dtype], device=t.device)
        self._launch("reduce_z", "aliby_reduce_z", _ptr(t), in_dtype, math.prod(lead), Z, Y * X, op, _ptr(out), out_dtype)
        return out

    # ------------------------------------------------------------------ objects
    def object_table(self, labels: torch.Tensor, max_labels=None) -> ObjectTable:
        """max_labels: the largest label of every frame when the caller knows it (the segmenter's object counts: its labels are
        1..n) — saves the pass over the label block that finds it and the host synchronisation behind that pass."""
        F, Y, X = labels.shape
        from aliby_amd import trace

        trace.mark("object_table:call")
        if max_labels is not None:
            mx = np.ascontiguousarray(max_labels, dtype=np.int32)
            if mx.shape != (F,) or (mx < 0).any():
                raise ValueError(f"max_labels must hold one non-negative count per frame ({F}), got shape {mx.shape}")
        else:
            mx = np.zeros(F, np.int32)
            self._launch("object_table", "aliby_label_max", _ptr(labels), F, Y, X, _ptr(mx))
        offsets = np.zeros(F + 1, np.int32)
        np.cumsum(mx, out=offsets[1:])
        n_obj = int(offsets[-1])
        host = np.zeros(n_obj, _lib.OBJECT_DTYPE)
        dev = torch.empty(max(n_obj, 1) * 32, dtype=torch.uint8, device=labels.device)
        if n_obj:
            self._launch("object_table", "aliby_object_table", _ptr(labels), F, Y, X, _ptr(offsets), _ptr(dev), _ptr(host))
        present = host["area"] > 0
        if present.any():
            hh = (host["y1"] - host["y0"])[present]
            ww = (host["x1"] - host["x0"])[present]
            max_area, max_h, max_w = int(host["area"].max()), int(hh.max()), int(ww.max())
        else:
            max_area = max_h = max_w = 0
        trace.mark("object_table:returned")
        return ObjectTable(dev, host, offsets, n_obj, max_area, max_h, max_w)

    def track_stitch(self, prev: torch.Tensor, cur: torch.Tensor, prev_table: ObjectTable, cur_table: ObjectTable,
                     prev_tracked: torch.Tensor | None, max_label: np.ndarray | None, threshold: float = 0.25):
        """IoU stitching of two label stacks [F,Y,X] (aliby_track_stitch).  Returns (tracked label per current object row
        as an int32 device tensor, new running maximum per tile as int32 [F])."""
        F, Y, X = cur.shape
        tracked = torch.zeros(max(cur_table.n_obj, 1), dtype=torch.int32, device=cur.device)
        mx_in = None if max_label is None else np.ascontiguousarray(max_label, dtype=np.int32)
        mx_out = np.zeros(F, np.int32)
        self._launch("track_stitch", "aliby_track_stitch", _ptr(prev), _ptr(cur), F, Y, X, _ptr(cur_table.dev), _ptr(cur_table.offsets),
                     _ptr(prev_table.dev), _ptr(prev_table.offsets), _ptr(prev_tracked), _ptr(mx_in), float(threshold), _ptr(tracked), _ptr(mx_out))
        return tracked[: cur_table.n_obj], mx_out

    # ----------------------------------------------------------------- Z-stacks as volumes (round 3 extension, BASELINE config 5)
    def stitch_planes(self, planes: torch.Tensor, counts=None, threshold: float = 0.01):
        """Per-plane label images of Z-stacks, uint16 [F,Z,Y,X] with labels 1..n per plane, -> (volume labels uint16 [F,Z,Y,X],
        objects per stack int32 [F]): cellpose's `stitch3D` along Z (the reference's do_3D branch passes stitch_threshold = 0.01,
        segment/dispatch.py:193-198) — plane z + 1 is stitched to the already stitched plane z by IoU (aliby_track_stitch, all F
        stacks per call), new labels continue from the stack's running maximum — then written back through a per-object table."""
        F, Z, Y, X = planes.shape
        zf = planes.permute(1, 0, 2, 3).contiguous()  # [Z,F,Y,X]: the planes of one z are consecutive tiles
        table = self.object_table(zf.view(Z * F, Y, X))
        off = table.offsets
        lut = torch.zeros(max(table.n_obj, 1), dtype=torch.int32, device=planes.device)
        # the stitcher takes F tiles per call: a row's tile index z * F + f becomes f (rows are 8 int32: tile, label, box, area)
        tab = table.dev.view(torch.int32).view(-1, 8).clone()
        tab[:, 0].remainder_(F)

        def rows(z):  # (table rows, rebased offsets) of the F planes at depth z
            lo, hi = int(off[z * F]), int(off[(z + 1) * F])
            return tab[lo: max(hi, lo + 1)], np.ascontiguousarray(off[z * F: (z + 1) * F + 1] - lo), lo, hi

        d0, o0, lo, hi = rows(0)
        if hi > lo:  # plane 0 keeps its own labels
            own = np.concatenate([np.arange(1, int(o0[f + 1] - o0[f]) + 1, dtype=np.int32) for f in range(F)]) if hi > lo else np.zeros(0, np.int32)
            lut[lo:hi] = torch.from_numpy(own).to(lut.device)
        mx = np.asarray([int(o0[f + 1] - o0[f]) for f in range(F)], np.int32)
        prev_rows, prev_off, prev_lo, prev_hi = d0, o0, lo, hi
        for z in range(1, Z):
            cur_rows, cur_off, lo, hi = rows(z)
            tracked = lut[lo: max(hi, lo + 1)]
            mx_out = np.zeros(F, np.int32)
            self._launch(None, "aliby_track_stitch", _ptr(zf[z - 1]), _ptr(zf[z]), F, Y, X, _ptr(cur_rows), _ptr(cur_off), _ptr(prev_rows),
                         _ptr(prev_off), _ptr(lut[prev_lo: max(prev_hi, prev_lo + 1)]), _ptr(np.ascontiguousarray(mx)), float(threshold),
                         _ptr(tracked), _ptr(mx_out))
            mx = mx_out
            prev_rows, prev_off, prev_lo, prev_hi = cur_rows, cur_off, lo, hi
        out = torch.empty_like(zf)
        self._launch(None, "aliby_labels_apply_lut", _ptr(zf), Z * F, Y, X, _ptr(np.ascontiguousarray(off)), _ptr(lut), _ptr(out))
        return out.permute(1, 0, 2, 3).contiguous(), mx

    @staticmethod
    def _volume_offsets(who: str, F: int, counts) -> np.ndarray:
        """counts [F] -> row offsets int32 [F + 1] of a volume method, as the C entries demand them (volume_offsets_ok)."""
        cnt = np.asarray(counts, np.int64).reshape(-1)
        if cnt.shape != (F,) or (cnt < 0).any() or (cnt > 65535).any():
            raise ValueError(f"{who}: counts must hold one label count (0..65535) per stack ({F}), got {counts!r}")
        offsets = np.zeros(F + 1, np.int32)
        np.cumsum(cnt, out=offsets[1:])
        return offsets

    @staticmethod
    def _volume_labels(who: str, volume):
        """Checks the labels of a volume method (uint16 [F,Z,Y,X] on the device) -> F, Z, Y, X."""
        if not isinstance(volume, torch.Tensor):
            raise TypeError(f"{who} takes torch tensors on the device")
        if volume.dtype != torch.uint16:
            raise TypeError(f"{who}: volume labels must be uint16, got {volume.dtype}")
        if volume.dim() != 4:
            raise ValueError(f"{who}: volume must be [F,Z,Y,X], got {tuple(volume.shape)}")
        if not volume.is_cuda:
            raise ValueError(f"{who} takes tensors on the device")
        return tuple(int(v) for v in volume.shape)

    @staticmethod
    def _volume_inputs(who: str, volume, pixels, counts):
        """Checks (volume uint16 [F,Z,Y,X], pixels uint16 or float32 [F,C,Z,Y,X], counts [F]) of a volume method -> F, C, Z, Y, X, offsets."""
        if not isinstance(pixels, torch.Tensor):
            raise TypeError(f"{who} takes torch tensors on the device")
        if pixels.dtype not in (torch.uint16, torch.float32):
            raise TypeError(f"{who}: pixels must be uint16 or float32, got {pixels.dtype}")
        F, Z, Y, X = FeatureEngine._volume_labels(who, volume)  # (after the pixels' types: a TypeError of either comes before any ValueError)
        if pixels.dim() != 5 or tuple(pixels.shape[:1]) != (F,) or tuple(pixels.shape[2:]) != (Z, Y, X):
            raise ValueError(f"{who}: volume must be [F,Z,Y,X] and pixels [F,C,Z,Y,X], got {tuple(volume.shape)} and {tuple(pixels.shape)}")
        if not pixels.is_cuda:
            raise ValueError(f"{who} takes tensors on the device")
        return F, int(pixels.shape[1]), Z, Y, X, FeatureEngine._volume_offsets(who, F, counts)

    @staticmethod
    def _integer(name: str, v) -> int:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an integer, got {v!r}")
        return int(v)

    @staticmethod
    def _channel(channel, Cn: int) -> int:
        channel = FeatureEngine._integer("channel", channel)
        if not 0 <= channel < Cn:
            raise ValueError(f"channel {channel} out of range for {Cn} channels")
        return channel

    @staticmethod
    def _pixel_code(pixels: torch.Tensor) -> int:
        """dtype code of the pixels of a volume method (uint16 or float32: _volume_inputs)."""
        return _lib.U16 if pixels.dtype == torch.uint16 else _lib.F32

    def _out_window(self, out, col0, rows: int, cols: int, what: str = "out", col0_name: str = "col0"):
        """-> (matrix, col0) to write a [rows, cols] result into: a new NaN matrix and 0, or the caller's `out` (float64
        [rows, >= col0 + cols] on the device, rows contiguous) and its col0 once they are checked (`what` names it in the refusal)."""
        if out is None:
            return self.new_output(rows, cols), 0
        col0 = self._integer(col0_name, col0)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or not out.is_cuda or out.dim() != 2:
            raise TypeError(f"{what} must be a float64 [rows, columns] tensor on the device")
        if out.shape[0] != rows or col0 < 0 or col0 + cols > out.shape[1] or (rows and out.stride(1) != 1):
            raise ValueError(f"{what} must hold {rows} rows and columns {col0}..{col0 + cols - 1} with unit column stride, got "
                             f"{tuple(out.shape)} with strides {tuple(out.stride())}")
        return out, col0

    def _volume_block(self, rows: int, cols: int, *launches, out=None, col0: int = 0) -> torch.Tensor:
        """The result of a volume method: a NaN block [rows, cols], written by every (profile group, entry, arguments) of `launches`
        in turn, where arguments((out, stride, col0)) gives the entry's arguments with that window in its place.  Stacks without any
        object: the empty block and no launch (found by tests/fuzz/fuzz_volume.py — the C entries refuse a NULL output).  With `out`
        (`_out_window`) the launches write out[:, col0 : col0 + cols] in place, and that view is returned: what
        extraction.families.evaluate_volume assembles its matrix with, instead of one block per family and a torch.cat.  Allocate
        `out` with `new_output` (NaN-filled): a family may leave the cells of a label without voxels as it found them."""
        given = out is not None
        out, col0 = self._out_window(out, col0, rows, cols)
        if rows:
            for group, entry, arguments in launches:
                with self.timed(group):  # around the arguments too: a copy to contiguous is part of the family's time
                    self._launch(None, entry, *arguments((_ptr(out), out.stride(0), col0)))
        return out[:, col0: col0 + cols] if given else out

    def intensity3d(self, volume: torch.Tensor, pixels: torch.Tensor, channel: int, counts, out=None, col0: int = 0) -> torch.Tensor:
        """Volume labels uint16 [F,Z,Y,X] (1..counts[f] per stack), pixels uint16 [F,C,Z,Y,X] -> float64 [sum counts, 12]
        (features.intensity3d_names(); aliby_features_intensity3d).  Rows in (stack, label) order.  A label of 1..counts[f]
        without voxels gets Volume 0 and NaN elsewhere; labels above counts[f] are not measured.  Exact 64-bit integer sums: bitwise
        independent of run and batch.  out, col0 (here and in every volume method): write the block into out[:, col0:] in place
        and return that view (`_volume_block`)."""
        F, Cn, Z, Y, X, offsets = self._volume_inputs("intensity3d", volume, pixels, counts)
        if pixels.dtype != torch.uint16:
            raise TypeError(f"intensity3d: pixels must be uint16 (the family has no float form), got {pixels.dtype}")
        channel = self._channel(channel, Cn)
        return self._volume_block(int(offsets[-1]), 12, ("intensity3d", "aliby_features_intensity3d", lambda o: (
            _ptr(volume.contiguous()), _ptr(pixels.contiguous()), F, Cn, Z, Y, X, channel, _ptr(offsets), *o)), out=out, col0=col0)

    @property
    def intensity3d_detail_lds_voxels(self) -> int:
        """Largest object, in voxels, that `intensity3d_detail` measures from LDS; larger ones go through global scratch (same results)."""
        return int(self.lib.aliby_intensity3d_detail_lds_voxels())

    def intensity3d_detail(self, volume: torch.Tensor, pixels: torch.Tensor, channel: int, counts, edge_measurements: bool = True, out=None,
                           col0: int = 0) -> torch.Tensor:
        """Volume labels uint16 [F,Z,Y,X] (1..counts[f] per stack), pixels uint16 or float32 [F,C,Z,Y,X] -> float64 [sum counts, 13]
        (8 with edge_measurements=False; features.intensity3d_detail_names(edge_measurements); aliby_features_intensity3d_detail): the
        columns of the 2-D `intensity` family that `intensity3d` lacks, over each object's voxels in raster order (z, y, x) — the five
        edge statistics (edge voxel: one of the six face neighbours inside the volume carries another value), MassDisplacement, the
        quartiles, median and MAD (CellProfiler's interpolation rule, float64), and the position of the maximum (ties to the last
        voxel in raster order).  torch.cat([intensity3d(...), intensity3d_detail(...)], 1) is the whole 2-D column set plus Volume and
        Location_Center_*.  Rows in (stack, label) order.  A label of 1..counts[f] without voxels gets a row of NaN (the edge columns
        too, where the 2-D family writes 0); an object with voxels but no edge voxel gets 0 in the edge columns; labels above counts[f]
        are not measured, but count as another value next to an object.  NaN pixels give unspecified results.  Objects above
        `intensity3d_detail_lds_voxels` voxels are measured in the context's scratch, where the object table is built too: a
        main-stream call, one in flight per context (the scratch rule, csrc/object_launch.h).  Bitwise independent of run and batch."""
        F, Cn, Z, Y, X, offsets = self._volume_inputs("intensity3d_detail", volume, pixels, counts)
        names = feat.intensity3d_detail_names(edge_measurements)  # (refuses a flag that is not a bool, before the channel's range)
        channel = self._channel(channel, Cn)
        return self._volume_block(int(offsets[-1]), len(names), ("intensity3d_detail", "aliby_features_intensity3d_detail", lambda o: (
            _ptr(volume.contiguous()), _ptr(pixels.contiguous()), self._pixel_code(pixels), F, Cn, Z, Y, X, channel, _ptr(offsets),
            int(edge_measurements), *o)), out=out, col0=col0)

    @staticmethod
    def _spacing3d(spacing) -> np.ndarray:
        sp = np.ascontiguousarray(np.asarray(spacing, np.float64).reshape(3))
        if not (np.isfinite(sp).all() and (sp > 0).all()):
            raise ValueError(f"spacing must be three positive finite numbers (dz, dy, dx), got {spacing!r}")
        return sp

    @staticmethod
    def surface3d_table(spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
        """The 256 per-cell areas behind `SurfaceArea` at a voxel size (dz, dy, dx) -> float64 [256] (aliby_surface3d_table):
        entry c is the area of the triangles scikit-image's Lewiner marching cubes at level 0 emits for a 2 x 2 x 2 cell whose voxel
        (z + dz, y + dy, x + dx) carries the label where bit 4 dz + 2 dy + dx of c is set.  Host arithmetic: needs no device."""
        sp = FeatureEngine._spacing3d(spacing)
        area = np.zeros(256, np.float64)
        _lib.check(_lib.load().aliby_surface3d_table(_ptr(sp), _ptr(area)))
        return area

    @staticmethod
    def _surface3d_shape(Z: int, Y: int, X: int) -> None:
        if min(int(Z), int(Y), int(X)) < 2:
            raise ValueError(f"SurfaceArea needs a volume of at least 2 x 2 x 2 voxels (a marching-cubes cell), got {(int(Z), int(Y), int(X))}")

    def sizeshape3d(self, volume: torch.Tensor, counts, spacing=(1.0, 1.0, 1.0), surface_area: bool = False, out=None, col0: int = 0) -> torch.Tensor:
        """Volume labels uint16 [F,Z,Y,X] (1..counts[f] per stack) -> float64 [sum counts, 19] (features.sizeshape3d_names();
        aliby_features_sizeshape3d).  Rows in (stack, label) order; spacing = physical voxel size (dz, dy, dx).  A label of
        1..counts[f] without voxels gets Volume 0 and NaN elsewhere, as in intensity3d.
        surface_area=True -> [sum counts, 20]: the same 19 columns from the same launch, and column 19 "SurfaceArea"
        (aliby_features_surface3d): the area of scikit-image's Lewiner marching-cubes mesh at level 0 of each object, as CellProfiler
        measures it, from exact per-object counts of the 2 x 2 x 2 cell configurations and `surface3d_table(spacing)`.  The mesh is
        open where an object touches a face of the volume; its vertices sit on the outside voxels' centres (one voxel: 4 sqrt(3)).
        An object that fills the whole volume gets 0 (scikit-image raises there); Z, Y, X must be at least 2."""
        F, Z, Y, X = self._volume_labels("sizeshape3d", volume)
        sp = self._spacing3d(spacing)
        if surface_area:
            self._surface3d_shape(Z, Y, X)
        offsets = self._volume_offsets("sizeshape3d", F, counts)
        volume = volume.contiguous()

        def launch(name, col):
            return name, "aliby_features_" + name, lambda o: (_ptr(volume), F, Z, Y, X, _ptr(offsets), _ptr(sp), o[0], o[1], o[2] + col)

        launches = [launch("sizeshape3d", 0)] + ([launch("surface3d", 19)] if surface_area else [])
        return self._volume_block(int(offsets[-1]), 20 if surface_area else 19, *launches, out=out, col0=col0)

    @property
    def coloc3d_lds_voxels(self) -> int:
        """Largest object, in voxels, that `coloc3d` measures from LDS; larger ones go through global scratch (same results)."""
        return int(self.lib.aliby_coloc3d_lds_voxels())

    def coloc3d(self, volume: torch.Tensor, pixels: torch.Tensor, pairs, counts, metrics=("pearson", "manders_fold", "rwc", "costes"),
                thr: float = 15.0, scale_max: float = 255.0, out=None, col0: int = 0) -> torch.Tensor:
        """Volume labels uint16 [F,Z,Y,X] (1..counts[f] per stack), pixels uint16 or float32 [F,C,Z,Y,X], pairs = [(c0, c1), ...]
        -> float64 [sum counts, 2 * len(metrics) * len(pairs)] (features.coloc3d_names(pairs, metrics); aliby_features_coloc3d):
        the 2-D colocalisation metrics over each object's voxels.  Rows in (stack, label) order, columns pair-major in the order
        of `pairs` and `metrics`.  A label of 1..counts[f] without voxels gets a row of NaN.  Bitwise independent of run and batch."""
        F, Cn, Z, Y, X, offsets = self._volume_inputs("coloc3d", volume, pixels, counts)
        names = feat.coloc3d_names(pairs, metrics)  # (refuses unknown or repeated metrics and malformed pairs)
        pr = np.ascontiguousarray(np.asarray([(int(a), int(b)) for a, b in pairs], np.int32).reshape(-1, 2))
        if len(pr) == 0 or len(pr) > 64:
            raise ValueError(f"coloc3d takes between 1 and 64 channel pairs per call, got {len(pr)}")
        if ((pr < 0) | (pr >= Cn)).any():
            raise ValueError(f"channel out of range for {Cn} channels: {pairs!r}")
        thr, scale_max = float(thr), float(scale_max)
        if not (np.isfinite(thr) and np.isfinite(scale_max) and scale_max > 0):
            raise ValueError(f"thr must be finite and scale_max positive and finite, got {thr!r}, {scale_max!r}")
        col = {m: 2 * k for k, m in enumerate(metrics)}
        return self._volume_block(int(offsets[-1]), len(names), ("coloc3d", "aliby_features_coloc3d", lambda o: (
            _ptr(volume.contiguous()), _ptr(pixels.contiguous()), self._pixel_code(pixels), F, Cn, Z, Y, X, _ptr(pr), len(pr), _ptr(offsets), *o,
            2 * len(metrics), col.get("pearson", -1), col.get("manders_fold", -1), col.get("rwc", -1), col.get("costes", -1), thr, scale_max)),
            out=out, col0=col0)

    @property
    def texture3d_lds_voxels(self) -> int:
        """Largest bounding box, in voxels, that `texture3d` measures from LDS; larger boxes go through global scratch (same results)."""
        return int(self.lib.aliby_texture3d_lds_voxels())

    def texture3d(self, volume: torch.Tensor, pixels: torch.Tensor, channel: int, counts, scale: int = 3, gray_levels: int = 256, out=None,
                  col0: int = 0) -> torch.Tensor:
        """Volume labels uint16 [F,Z,Y,X] (1..counts[f] per stack), pixels uint16 or float32 [F,C,Z,Y,X] -> float64 [sum counts, 169]
        (features.texture3d_names(scale, gray_levels); aliby_features_texture3d): the 13 Haralick statistics of the 2-D `texture`
        in 13 directions over each object's bounding box, direction-major.  Rows in (stack, label) order.  A direction without a
        voxel pair gets 13 NaN, a label of 1..counts[f] without voxels a row of NaN.  Bitwise independent of run and batch."""
        F, Cn, Z, Y, X, offsets = self._volume_inputs("texture3d", volume, pixels, counts)
        scale, gray_levels = self._integer("scale", scale), self._integer("gray_levels", gray_levels)
        channel = self._channel(channel, Cn)
        if scale < 1 or not 2 <= gray_levels <= 256:
            raise ValueError(f"texture3d needs scale >= 1 and 2 <= gray_levels <= 256, got {scale}, {gray_levels}")
        cols = len(feat.texture3d_names(scale, gray_levels))
        return self._volume_block(int(offsets[-1]), cols, ("texture3d", "aliby_features_texture3d", lambda o: (
            _ptr(volume.contiguous()), _ptr(pixels.contiguous()), self._pixel_code(pixels), F, Cn, Z, Y, X, channel, _ptr(offsets), scale, gray_levels,
            *o)), out=out, col0=col0)

    def neighbors3d(self, volume: torch.Tensor, counts, distance=None, out=None, col0: int = 0) -> torch.Tensor:
        """Volume labels uint16 [F,Z,Y,X] (1..counts[f] per stack) -> float64 [sum counts, 7] (features.neighbors3d_names(distance);
        aliby_features_neighbors3d): the `neighbors` family on volumes — the number of objects within `distance` voxels, the share of
        the plane-by-plane outline in contact with them, the two closest objects of the stack by centre, and the angle between them.
        Rows in (stack, label) order.  distance=None: adjacent objects (d = 1); else an integer in 1..16 (ValueError otherwise; the cap
        bounds the per-voxel scan, it is not a structural limit).  A label of 1..counts[f] without voxels gets a row of NaN; values
        above counts[f] touch but are neither counted nor measured.  Voxel spacing is not used.  PARITY UNPINNED, and the angle is
        atan2(|v1 x v2|, v1 . v2) where CellProfiler takes an arccos: the definition, and what is not built ("Expand until adjacent", a
        second object set, physical-unit balls), are in include/aliby_hip.h.  The object table is built in the context's scratch: a
        main-stream call.  Bitwise independent of run and batch."""
        d = feat.neighbors3d_distance(distance)
        F, Z, Y, X = self._volume_labels("neighbors3d", volume)
        offsets = self._volume_offsets("neighbors3d", F, counts)
        centres = torch.empty((int(offsets[-1]), 3), dtype=torch.float64, device=volume.device)
        return self._volume_block(int(offsets[-1]), 7, ("neighbors3d", "aliby_features_neighbors3d", lambda o: (
            _ptr(volume.contiguous()), F, Z, Y, X, _ptr(offsets), d, _ptr(centres), *o)), out=out, col0=col0)

    @staticmethod
    def _granularity3d_shapes(Z: int, Y: int, X: int, subsample_size: float, image_sample_size: float):
        """-> the subsampled and the background shape of `granularity3d`: ceil(n * size) per axis when the size is below 1, else n
        (numpy's mgrid[0 : n * size] has that many points)."""
        sub = tuple(int(np.ceil(n * subsample_size)) if subsample_size < 1 else int(n) for n in (Z, Y, X))
        return sub, tuple(int(np.ceil(n * image_sample_size)) if image_sample_size < 1 else n for n in sub)

    def granularity3d(self, volume: torch.Tensor, pixels: torch.Tensor, channel: int, counts, subsample_size: float = 0.25,
                      image_sample_size: float = 0.25, element_size: int = 10, granular_spectrum_length: int = 16, out=None,
                      col0: int = 0) -> torch.Tensor:
        """Volume labels uint16 [F,Z,Y,X] (1..counts[f] per stack), pixels uint16 or float32 [F,C,Z,Y,X] -> float64 [sum counts, L]
        (features.granularity3d_names(L); aliby_features_granularity3d): the `granularity` family on volumes, CellProfiler
        MeasureGranularity's volumetric branch — each stack of `channel` subsampled trilinearly by `subsample_size`, its background
        (grey erosion and dilation with ball(element_size) on a further `image_sample_size` subsample, resized back) removed, then L
        rounds of erosion by ball(1) and reconstruction by dilation; Granularity_i = (mean_{i-1} - mean_i) * 100 / max(mean_0, eps)
        over each object's voxels, mean_0 on the original pixels.  The image mask is the whole stack (CellProfiler's default).  Where
        the destination axis of a resize has length 1 its coordinate is 0 (CellProfiler divides 0 by 0 there): with this one
        departure a stack of one plane is the 2-D `granularity`.  Rows in (stack, label) order.  A label of 1..counts[f] without
        voxels gets a row of NaN; labels above counts[f] are not measured.  Y, X and their two sampled lengths must be above 1, Z may
        be 1; element_size is an integer in 1..16 (the cap bounds the per-voxel scan of the ball, it is not a structural limit), L
        in 1..64.  PARITY UNPINNED: the definition is in include/aliby_hip.h, restated in tests/granularity3d_ref.py.  The
        reconstruction reads a change flag every 16 sweeps, so the call waits on its stream: a main-stream call.  `granularity3d_sweeps`
        holds the sweeps of each spectrum step of the last call.  Bitwise independent of run and batch."""
        F, Cn, Z, Y, X, offsets = self._volume_inputs("granularity3d", volume, pixels, counts)
        channel = self._channel(channel, Cn)
        sizes = []
        for name, v in (("subsample_size", subsample_size), ("image_sample_size", image_sample_size)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (np.isfinite(v) and 0 < v <= 1):
                raise ValueError(f"granularity3d: {name} must be a finite number in (0, 1], got {v!r}")
            sizes.append(float(v))
        element_size, L = self._integer("element_size", element_size), self._integer("granular_spectrum_length", granular_spectrum_length)
        if not 1 <= element_size <= feat.GRANULARITY3D_MAX_ELEMENT:
            raise ValueError(f"granularity3d: element_size must lie in 1..{feat.GRANULARITY3D_MAX_ELEMENT}, got {element_size}")
        names = feat.granularity3d_names(L)  # (refuses a length outside 1..64)
        sub, back = self._granularity3d_shapes(Z, Y, X, *sizes)
        if min(Y, X, *sub[1:], *back[1:]) <= 1:
            raise ValueError(f"granularity3d: Y, X and their sampled lengths must be above 1, got a stack {(Z, Y, X)}, subsampled {sub}, background {back}")
        rows = int(offsets[-1])
        sweeps = np.zeros(L, np.int32)

        def arguments(o):
            need = int(self.lib.aliby_granularity3d_workspace_bytes(F, Z, Y, X, rows, sizes[0], sizes[1]))
            work = torch.empty((need + 7) // 8, dtype=torch.float64, device=volume.device)
            return (_ptr(volume.contiguous()), _ptr(pixels.contiguous()), self._pixel_code(pixels), F, Cn, Z, Y, X, channel, _ptr(offsets),
                    sizes[0], sizes[1], element_size, L, _ptr(work), work.numel() * 8, _ptr(sweeps), *o)

        block = self._volume_block(rows, len(names), ("granularity3d", "aliby_features_granularity3d", arguments), out=out, col0=col0)
        self.granularity3d_sweeps = sweeps.tolist()
        return block

    def projection3d(self, volume: torch.Tensor, counts, out=None, col0: int = 0) -> torch.Tensor:
        """Volume labels uint16 [F,Z,Y,X] (1..counts[f] per stack) -> float64 [sum counts, 4] (features.projection3d_names();
        aliby_features_projection3d): how the collapse of the stack to 2-D — the maximum over z, then a sequential relabel
        (`segment.model.max_project_and_relabel`, what a 3-D segment step returns) — sees each object.  With `top` the maximum over z
        of a column (y, x): Projection_Area = columns holding a voxel of the object (a label that re-enters a column counts once),
        Projection_VisibleArea = columns whose top it is, Projection_VisibleFraction = their float64 quotient, Projection_Label = the
        object's label in the collapsed image (the rank of its value among the values that are top somewhere), 0 when it is hidden
        everywhere.  Rows in (stack, label) order.  A value above counts[f] gets no row but occludes and counts in the rank; a
        label of 1..counts[f] without voxels gets 0, 0, NaN, 0.  One read of the labels.  The counts and the per-stack presence
        bits live in the context's scratch: a main-stream call, one in flight per context (the scratch rule,
        csrc/object_launch.h).  Integers and one division: bitwise independent of run and batch."""
        F, Z, Y, X = self._volume_labels("projection3d", volume)
        offsets = self._volume_offsets("projection3d", F, counts)
        return self._volume_block(int(offsets[-1]), 4, ("projection3d", "aliby_features_projection3d", lambda o: (
            _ptr(volume.contiguous()), F, Z, Y, X, _ptr(offsets), *o)), out=out, col0=col0)

    def relabel_sequential(self, labels: torch.Tensor) -> np.ndarray:
        F, Y, X = labels.shape
        n = np.zeros(F, np.int32)
        self._launch(None, "aliby_relabel_sequential", _ptr(labels), F, Y, X, _ptr(n))
        return n

    # ----------------------------------------------------------------- features
    def new_output(self, n_obj: int, n_cols: int) -> torch.Tensor:
        return torch.full((max(n_obj, 1), max(n_cols, 1)), float("nan"), dtype=torch.float64, device=f"cuda:{self.device}")[:n_obj]

    @staticmethod
    def _head(labels, planes, dtype, channel, raw_code: bool = False, pixels: bool = True) -> tuple:
        """(labels, planes, dtype code, F, Cn, Y, X, channel): how the per-channel entries begin.  F, Y, X are the planes' [F,C,Y,X],
        and the labels' where there are none (planes=None: a null pointer, no channels, channel 0).  raw_code: the code as the
        caller gave it, U8W included (texture alone tells it from U16: `_kdt`).  pixels=False: the mask-only form, where the
        planes are there but not looked at (null pointer, code 0, channel 0)."""
        if planes is None:
            (F, Y, X), Cn = labels.shape, 0
        else:
            F, Cn, Y, X = planes.shape
        if not pixels:
            return _ptr(labels), 0, 0, F, Cn, Y, X, 0
        code = dtype if raw_code or dtype != _lib.U8W else _lib.U16  # (`_kdt`, spelled out: this runs once per launch)
        return _ptr(labels), _ptr(planes), code, F, Cn, Y, X, 0 if planes is None else int(channel)

    @staticmethod
    def _row_stride(out, rows: int, col0: int, cols: int) -> int:
        """The row stride handed to C for columns col0..col0+cols-1 of `out`: a matrix without rows has none of its own."""
        return out.stride(0) if rows else max(col0 + cols, 1)

    @staticmethod
    def _relate_out(out, rows: int) -> tuple:
        """(pointer, row stride) of one side of `relate` / `relate3d`: a side without rows is handed over as (NULL, 5)."""
        return (_ptr(out), out.stride(0)) if rows else (0, 5)

    def intensity(self, labels, planes, dtype, channel, table: ObjectTable, out, col0, edge_measurements=True):
        self._launch("intensity", "aliby_features_intensity", *self._head(labels, planes, dtype, channel), _ptr(table.dev), table.n_obj,
                     table.max_area, 1 if edge_measurements else 0, _ptr(out), out.stride(0), col0)
        return len(feat.intensity_names(edge_measurements))

    def sizeshape(self, labels, table: ObjectTable, out, col0):
        F, Y, X = labels.shape
        self._launch("sizeshape", "aliby_features_sizeshape", _ptr(labels), F, Y, X, _ptr(table.dev), table.n_obj, table.max_h, table.max_w,
                     table.max_area, _ptr(out), out.stride(0), col0)
        return 78

    def feret(self, labels, table: ObjectTable, out, col0):
        F, Y, X = labels.shape
        self._launch("feret", "aliby_features_feret", _ptr(labels), F, Y, X, _ptr(table.dev), table.n_obj, table.max_h, _ptr(out),
                     out.stride(0), col0)
        return 2

    def mec(self, labels, table: ObjectTable) -> torch.Tensor:
        """Minimum enclosing circles [n_obj,4], computed once per object table."""
        if table._mec is None:
            F, Y, X = labels.shape
            mec = torch.empty((max(table.n_obj, 1), 4), dtype=torch.float64, device=labels.device)
            self._launch("mec", "aliby_object_mec", _ptr(labels), F, Y, X, _ptr(table.dev), table.n_obj, table.max_h, _ptr(mec))
            table._mec = mec
        return table._mec

    def neighbors(self, labels, table: ObjectTable, out, col0, distance=None):
        """Columns col0..col0+6 of out [n_obj, .]: the `neighbors` family (features.neighbors_names(distance);
        aliby_features_neighbors) — CellProfiler's MeasureObjectNeighbors with the objects as their own neighbours: the number of
        neighbours within `distance` pixels, the share of the outline in contact with them, the two closest objects by centre, and the
        angle between them.  distance=None: adjacent objects (d = 1); else an integer in 1..64 (ValueError otherwise).  PARITY
        UNPINNED, and the angle is atan2(|v1 x v2|, v1 . v2) where CellProfiler takes an arccos: the definition, and what is not built
        ("Expand until adjacent", a second object set), are in include/aliby_hip.h.  Uses no context scratch."""
        d = feat.neighbors_distance(distance)
        F, Y, X = labels.shape
        if table.n_obj == 0:
            return 7
        centres = torch.empty((table.n_obj, 2), dtype=torch.float64, device=labels.device)
        self._launch("neighbors", "aliby_features_neighbors", _ptr(labels), F, Y, X, _ptr(table.dev), table.n_obj, table.max_h, table.max_w,
                     _ptr(self._offsets_dev(table, labels.device)), int(np.diff(table.offsets).max()), d, _ptr(centres), _ptr(out),
                     out.stride(0), col0)
        return 7

    @staticmethod
    def _offsets_dev(table: ObjectTable, device) -> torch.Tensor:
        """The table's row offsets int32 [F + 1] on the device, copied there once per table."""
        if table._offsets_dev is None:
            table._offsets_dev = torch.from_numpy(np.ascontiguousarray(table.offsets, dtype=np.int32)).to(device)
        return table._offsets_dev

    @staticmethod
    def _label_blocks(who: str, dims: str, blocks: dict, together: str | None = None, typed: bool = True, got: bool = True) -> tuple:
        """Checks the label blocks {name: tensor} of a relate, tertiary or secondary method -> their shape.  typed: each is a uint16
        [dims] tensor on the device (`got`: the refusal says what came instead); `together` (how the refusal names them): all have
        one shape of that rank.  Every refusal is a ValueError (`_volume_labels`, the feature families' check, raises TypeError)."""
        rank = dims.count(",") + 1
        for name, v in blocks.items() if typed else ():
            if not isinstance(v, torch.Tensor) or v.dtype != torch.uint16 or v.dim() != rank or not v.is_cuda:
                what = f", got {(v.dtype, tuple(v.shape)) if isinstance(v, torch.Tensor) else type(v).__name__}" if got else ""
                raise ValueError(f"{who}: {name} must be a uint16 [{dims}] tensor on the device{what}")
        first, *rest = blocks.values()
        if any(tuple(v.shape) != tuple(first.shape) for v in rest) or first.ndim != rank:
            raise ValueError(f"{who}: {together} must share one shape [{dims}], got {' and '.join(str(tuple(v.shape)) for v in blocks.values())}")
        return tuple(int(n) for n in first.shape)

    def relate(self, labels_a, table_a: ObjectTable, labels_b, table_b: ObjectTable, out_a=None, col0_a=0, out_b=None, col0_b=0):
        """Two label blocks uint16 [F,Y,X] of one shape with their object tables -> (matrix_a, matrix_b), float64 [n, 5] each: the rows
        of A relative to B and of B relative to A (features.relate_names(other); aliby_features_relate) — CellProfiler's RelateObjects:
        the parent (most shared pixels, ties to the smaller label, 0 = none), that overlap, the number of children, the distance
        between the centres and from the centre to the parent's outline (NaN without a parent).  out_a / out_b: matrices [n, .] to
        write columns col0..col0+4 of instead of new ones (the returned matrix is then that window).  Differing F, Y or X is a
        ValueError.  PARITY UNPINNED; the definition and what is not built are in include/aliby_hip.h.  May use the context's scratch
        (tiles of more than 8191 labels)."""
        F, Y, X = self._label_blocks("relate", "F,Y,X", {"labels_a": labels_a, "labels_b": labels_b}, "the two label blocks", typed=False)
        if len(table_a.offsets) != F + 1 or len(table_b.offsets) != F + 1:
            raise ValueError(f"relate: the object tables are not those of {F} tiles")
        if out_a is None:
            out_a, col0_a = self.new_output(table_a.n_obj, 5), 0
        if out_b is None:
            out_b, col0_b = self.new_output(table_b.n_obj, 5), 0
        if table_a.n_obj or table_b.n_obj:
            # (a multiple of 8 bytes; float64 elements keep it 8-byte aligned)
            work = torch.empty(int(self.lib.aliby_relate_workspace_bytes(table_a.n_obj, table_b.n_obj)) // 8, dtype=torch.float64,
                               device=labels_a.device)
            self._launch("relate", "aliby_features_relate", _ptr(labels_a), _ptr(labels_b), F, Y, X,
                         _ptr(table_a.dev), table_a.n_obj, table_a.max_h, table_a.max_w, _ptr(table_b.dev), table_b.n_obj, table_b.max_h, table_b.max_w,
                         _ptr(self._offsets_dev(table_a, labels_a.device)), int(np.diff(table_a.offsets).max()),
                         _ptr(self._offsets_dev(table_b, labels_b.device)), int(np.diff(table_b.offsets).max()), _ptr(work),
                         *self._relate_out(out_a, table_a.n_obj), col0_a, *self._relate_out(out_b, table_b.n_obj), col0_b)
        return out_a[:, col0_a:col0_a + 5], out_b[:, col0_b:col0_b + 5]

    def tertiary_labels(self, outer, inner, shrink_inner: bool = True) -> torch.Tensor:
        """outer, inner uint16 [F,Y,X] of one shape -> device uint16 [F,Y,X] (aliby_tertiary_labels): outer's labels where inner is 0
        or, with shrink_inner, on the outline of an inner object; 0 elsewhere — CellProfiler's IdentifyTertiaryObjects (the cytoplasm
        = cell minus nucleus).  Labels keep outer's numbering; one that loses every pixel is absent.  PARITY UNPINNED
        (include/aliby_hip.h)."""
        F, Y, X = self._label_blocks("tertiary_labels", "F,Y,X", {"outer": outer, "inner": inner}, "outer and inner", typed=False)
        out = torch.empty_like(outer)
        if out.numel():
            self._launch("tertiary", "aliby_tertiary_labels", _ptr(outer), _ptr(inner), F, Y, X, 1 if shrink_inner else 0, _ptr(out))
        return out

    def secondary_labels(self, primary, distance) -> torch.Tensor:
        """primary uint16 [F,Y,X] on the device -> device uint16 [F,Y,X] (aliby_secondary_labels): CellProfiler's
        IdentifySecondaryObjects, method "Distance - N" (skimage's expand_labels) — every object grows by up to `distance` pixels into
        the background, each grown pixel taking the label of the nearest labelled pixel of its tile by exact integer squared distance,
        ties to the smaller label (SciPy's choice on a tie follows its sweep order).  Labels keep the primary numbering, so a secondary
        row joins its primary on the label; nothing crosses a tile edge.  `distance`: an integer in 1..64.  A tensor that is not
        uint16 [F,Y,X] on the device, and a bad distance, are ValueErrors.  Integer arithmetic: the same bits whatever the batch and
        the stream.  Uses no context scratch (its 4-bytes-per-pixel workspace is allocated here)."""
        n = feat.secondary_distance(distance)
        F, Y, X = self._label_blocks("secondary_labels", "F,Y,X", {"primary": primary})
        primary = primary.contiguous()
        out = torch.empty_like(primary)
        if out.numel():
            nbytes = int(self.lib.aliby_secondary_workspace_bytes(F, Y, X))
            work = torch.empty(nbytes // 4, dtype=torch.int32, device=primary.device)
            self._launch("secondary", "aliby_secondary_labels", _ptr(primary), F, Y, X, n, _ptr(work), nbytes, _ptr(out))
        return out

    def secondary_volume(self, primary, distance, spacing=(1, 1, 1)) -> torch.Tensor:
        """primary uint16 [F,Z,Y,X] on the device -> device uint16 [F,Z,Y,X] (aliby_secondary_volume): `secondary_labels` on volume
        labels — every object of a stack grows by up to `distance` into the background, a grown voxel taking the label of the nearest
        labelled voxel of its stack by the exact integer squared distance (sz dz)^2 + (sy dy)^2 + (sx dx)^2, ties to the smaller label
        (scipy's distance_transform_edt with sampling=spacing and its index gather, except on ties).  `distance`: an integer in 1..255
        in the units of `spacing` = (sz, sy, sx), three integers in 1..255, with distance // s at most 64 on every axis
        (features.secondary_volume_args).  Labels keep the primary numbering and the counts: no object can vanish.  With Z == 1 and
        unit spacing it carries the bits of `secondary_labels`.  A tensor that is not uint16 [F,Z,Y,X] on the device, a bad distance
        and a bad spacing are ValueErrors.  Integer arithmetic: the same bits whatever the batch and the stream.  Uses no context
        scratch (its 8-bytes-per-voxel workspace is allocated here)."""
        n, (sz, sy, sx) = feat.secondary_volume_args(distance, spacing)
        F, Z, Y, X = self._label_blocks("secondary_volume", "F,Z,Y,X", {"primary": primary})
        primary = primary.contiguous()
        out = torch.empty_like(primary)
        if out.numel():
            nbytes = int(self.lib.aliby_secondary_volume_workspace_bytes(F, Z, Y, X))
            work = torch.empty(nbytes // 4, dtype=torch.int32, device=primary.device)
            self._launch("secondary3d", "aliby_secondary_volume", _ptr(primary), F, Z, Y, X, n, sz, sy, sx, _ptr(work), nbytes, _ptr(out))
        return out

    def auto_threshold(self, image, method="otsu", classes=2, middle=None, correction=1.0, bounds=(0, 65535), return_details=False):
        """image uint16 [F,Y,X] on the device -> device int32 [F] (aliby_auto_threshold), with return_details (thresholds, details
        int32 [F,4] = (lo, hi, t1, t2) raw): Otsu's threshold of every tile on its own, over all its pixels — CellProfiler's automatic
        threshold for IdentifySecondaryObjects.  Two classes: the smallest grey level t that maximises s0^2/n0 + s1^2/n1 over the
        classes {v < t}, {v >= t} of the 65 536-level histogram.  Three classes: the same criterion over pairs of 256 bins of the
        occupied range lo..hi; middle="foreground" (the default) takes the lower threshold, "background" the upper.  Then
        min(max(rint(t * correction), bounds[0]), bounds[1]).  The arguments are those of features.auto_threshold_args.  The result
        stays on the device: propagate_labels(thresholds=...) reads it there.  A tensor that is not uint16 [F,Y,X] on the device is a
        ValueError; a float32 image is refused by name; views need not be contiguous.  Exact integers and correctly rounded float64:
        the same bits whatever the batch and the stream, equal to tests/threshold_ref.py.  PARITY UNPINNED (include/aliby_hip.h).
        Stream-ordered: no wait, no context scratch (its 256 KiB-per-tile histogram is allocated here)."""
        args = feat.auto_threshold_args(method, classes, middle, correction, bounds)
        if isinstance(image, torch.Tensor) and image.dtype == torch.float32:
            raise ValueError("auto_threshold: a float32 image is not built (the histogram is over uint16 grey levels): pass the uint16 pixels")
        F, Y, X = self._label_blocks("auto_threshold", "F,Y,X", {"image": image})
        if F > 65535 or Y * X >= 1 << 32:
            raise ValueError(f"auto_threshold: at most 65535 tiles of fewer than 2^32 pixels in one call, got {F} of {Y} x {X}")
        image = image.contiguous()
        out = torch.zeros(F, dtype=torch.int32, device=image.device)
        details = torch.zeros((F, 4), dtype=torch.int32, device=image.device) if return_details else None
        if image.numel():
            nbytes = int(self.lib.aliby_auto_threshold_workspace_bytes(F))
            work = torch.empty(nbytes // 4, dtype=torch.int32, device=image.device)
            self._launch("auto_threshold", "aliby_auto_threshold", _ptr(image), F, Y, X, args.classes,
                         args.middle_code, args.correction, args.bounds[0], args.bounds[1], _ptr(work), nbytes,
                         _ptr(out), _ptr(details) if details is not None else None)
        return (out, details) if return_details else out

    def propagate_labels(self, primary, image, threshold=0, regularization=0.05, distance=None, image_max=65535, return_distances=False,
                         thresholds=None):
        """primary, image uint16 [F,Y,X] on the device -> device uint16 [F,Y,X] (aliby_propagate_labels), with return_distances
        (labels, D uint64 [F,Y,X]): CellProfiler's IdentifySecondaryObjects, method "Propagation" — the primary labels grow along the
        stain `image`.  A pixel is passable if it is labelled, or image >= threshold and (with `distance`) within that many pixels
        of a labelled pixel; a step between 8-neighbours costs isqrt(256 (P^2 + m lambda2)) sixteenths of a grey level, P the summed
        absolute differences of the two 3 x 3 neighbourhoods (coordinates clamped to the tile), m = 1 straight and 2 diagonal; a pixel
        takes the label of the cheapest path, ties to the smaller label, 0 (and D = 2^64 - 1) where none arrives.  The arguments are
        those of features.propagate_args; "Distance - B" is threshold=0 with a distance.  Labels keep the primary numbering; nothing
        crosses a tile edge; a tile may hold at most 2^23 pixels.  Tensors that are not uint16 [F,Y,X] on the device and of one
        shape are ValueErrors; a float32 image is refused by name.  Exact integers: the same bits whatever the batch and the stream.
        PARITY UNPINNED (include/aliby_hip.h).  Waits on the stream between chunks of rounds; `propagate_stats` keeps the last call's
        (rounds that changed a key, flag reads).  Uses no context scratch (its 32-bytes-per-pixel workspace is allocated here).
        `thresholds`: a device int32 [F] tensor with one threshold per tile in place of `threshold` (auto_threshold's result, read
        on the device: aliby_propagate_labels_per_tile); a value above 65535 lets no unlabelled pixel of its tile pass.  Together
        with a non-zero `threshold`, or of another dtype, shape or device, it is a ValueError."""
        args = feat.propagate_args(threshold, regularization, distance, image_max)
        if thresholds is not None and args.threshold != 0:
            raise ValueError(f"propagate_labels: give threshold or thresholds, not both (threshold={threshold!r})")
        thr, n, lambda2 = args.threshold, args.distance, args.lambda2
        if isinstance(image, torch.Tensor) and image.dtype == torch.float32:
            raise ValueError("propagate_labels: a float32 image is not built (the metric is an exact integer on uint16 grey levels): "
                             "pass the uint16 pixels")
        F, Y, X = self._label_blocks("propagate_labels", "F,Y,X", {"primary": primary, "image": image}, "primary and image")
        if Y * X > 1 << 23:
            raise ValueError(f"propagate_labels: a tile may hold at most 2^23 pixels, got {Y} x {X}")
        if thresholds is not None:
            if not isinstance(thresholds, torch.Tensor) or thresholds.dtype != torch.int32 or tuple(thresholds.shape) != (F,) \
                    or thresholds.device != primary.device:
                got = (thresholds.dtype, tuple(thresholds.shape), str(thresholds.device)) if isinstance(thresholds, torch.Tensor) \
                    else type(thresholds).__name__
                raise ValueError(f"propagate_labels: thresholds must be an int32 [{F}] tensor on the device of the labels, got {got}")
            thresholds = thresholds.contiguous()
        primary, image = primary.contiguous(), image.contiguous()
        out = torch.empty_like(primary)
        dist = torch.empty(primary.shape, dtype=torch.uint64, device=primary.device) if return_distances else None
        stats = np.zeros(2, np.int32)
        if out.numel():
            nbytes = int(self.lib.aliby_propagate_workspace_bytes(F, Y, X))
            work = torch.empty(nbytes // 8, dtype=torch.int64, device=primary.device)
            entry, level = ("aliby_propagate_labels", thr) if thresholds is None else ("aliby_propagate_labels_per_tile", _ptr(thresholds))
            self._launch("propagate", entry, _ptr(primary), _ptr(image), F, Y, X, level, lambda2, n or 0, _ptr(work), nbytes,
                         _ptr(out), _ptr(dist) if dist is not None else None, _ptr(stats))
        self.propagate_stats = (int(stats[0]), int(stats[1]))
        return (out, dist) if return_distances else out

    def relate3d(self, volume_a, counts_a, volume_b, counts_b, spacing=(1.0, 1.0, 1.0), out_a=None, col0_a=0, out_b=None, col0_b=0):
        """Two sets of volume labels uint16 [F,Z,Y,X] of one shape (1..counts_*[f] per stack) -> (matrix_a, matrix_b), float64
        [sum counts, 5] each, rows in (stack, label) order: the rows of A relative to B and of B relative to A
        (features.relate3d_names(other); aliby_features_relate3d) — the `relate` family on volumes: the parent (most shared voxels, ties
        to the smaller label, 0 = none), that overlap, the number of children, the distance between the centres and from the centre to
        the parent's plane-by-plane outline (NaN without a parent), in the units of `spacing` = (dz, dy, dx), positive and finite.  On
        a stack of one plane with unit spacing every column carries the bits of `relate`.  out_a / out_b: matrices [rows, .] to write
        columns col0..col0+4 of instead of new ones (the returned matrix is then that window).  An empty set gives a [0, 5] matrix, and
        the other side's rows then have no parent and no children.  Volumes that are not uint16 [F,Z,Y,X] of one shape, counts of
        the wrong length and a bad spacing are ValueErrors.  PARITY UNPINNED; the definition is in include/aliby_hip.h.  The object
        tables and the counters live in the context's scratch: a main-stream call.  Bitwise independent of run, batch and launch form."""
        F, Z, Y, X = self._label_blocks("relate3d", "F,Z,Y,X", {"volume_a": volume_a, "volume_b": volume_b}, "the two volumes")
        sp = self._spacing3d(spacing)
        off_a, off_b = self._volume_offsets("relate3d (counts_a)", F, counts_a), self._volume_offsets("relate3d (counts_b)", F, counts_b)
        n_a, n_b = int(off_a[-1]), int(off_b[-1])
        out_a, col0_a = self._out_window(out_a, col0_a, n_a, 5, "relate3d: out_a", "col0_a")
        out_b, col0_b = self._out_window(out_b, col0_b, n_b, 5, "relate3d: out_b", "col0_b")
        if (n_a or n_b) and volume_a.numel():
            va, vb = volume_a.contiguous(), volume_b.contiguous()
            self._launch("relate3d", "aliby_features_relate3d", _ptr(va), _ptr(vb), F, Z, Y, X, _ptr(off_a), _ptr(off_b), _ptr(sp),
                         *self._relate_out(out_a, n_a), col0_a, *self._relate_out(out_b, n_b), col0_b)
        return out_a[:, col0_a:col0_a + 5], out_b[:, col0_b:col0_b + 5]

    def tertiary_volume(self, outer, inner, shrink_inner: bool = True) -> torch.Tensor:
        """outer, inner uint16 [F,Z,Y,X] of one shape -> device uint16 [F,Z,Y,X]: outer's labels where inner is 0 or, with
        shrink_inner, on the plane-by-plane outline of an inner object; 0 elsewhere — the tertiary image of every plane
        (aliby_tertiary_labels on the [F Z, Y, X] view: the outline of a volume is taken plane by plane, so no other kernel is
        needed).  It keeps outer's labels and counts; a label that loses every voxel is absent.  At a nucleus's top and bottom caps
        only the cap's in-plane rim is kept.  PARITY UNPINNED (include/aliby_hip.h)."""
        F, Z, Y, X = self._label_blocks("tertiary_volume", "F,Z,Y,X", {"outer": outer, "inner": inner}, "outer and inner", got=False)
        planes = self.tertiary_labels(outer.contiguous().view(F * Z, Y, X), inner.contiguous().view(F * Z, Y, X), shrink_inner=shrink_inner)
        return planes.view(F, Z, Y, X)

    def zernike(self, labels, planes, dtype, channel, table: ObjectTable, out, col0, weighted: bool):
        mec = self.mec(labels, table)
        self._launch("radial_zernikes" if weighted else "zernike", "aliby_features_zernike",
                     *self._head(labels, planes, dtype, channel, pixels=weighted), _ptr(table.dev), table.n_obj, _ptr(mec),
                     1 if weighted else 0, _ptr(out), out.stride(0), col0)
        return 60 if weighted else 30

    def radial_zernikes_multi(self, labels, planes, dtype, channels, table: ObjectTable, out, col0s):
        """radial_zernikes of several channels of one plane block: launches of up to five channels share the channel-independent
        basis (aliby_features_radial_zernikes_multi); a channel left alone goes through `zernike(weighted=True)`."""
        mec = self.mec(labels, table)
        channels, col0s = list(map(int, channels)), list(map(int, col0s))
        k = 0
        while k < len(channels):
            n = min(5, len(channels) - k)
            if len(channels) - k - n == 1:  # never leave a single channel for the last launch
                n -= 1
            if n == 1:
                self.zernike(labels, planes, dtype, channels[k], table, out, col0s[k], True)
            else:
                ch = (C.c_int * n)(*channels[k : k + n])
                c0 = (C.c_int * n)(*col0s[k : k + n])
                self._launch("radial_zernikes", "aliby_features_radial_zernikes_multi", *self._head(labels, planes, dtype, 0)[:7], ch, c0, n,
                             _ptr(table.dev), table.n_obj, _ptr(mec), _ptr(out), out.stride(0))
            k += n
        return 60

    def texture(self, labels, planes, dtype, channel, table: ObjectTable, out, col0, scale=3, gray_levels=256):
        self._launch("texture", "aliby_features_texture", *self._head(labels, planes, dtype, channel, raw_code=True), _ptr(table.dev),
                     table.n_obj, table.max_h, table.max_w, table.max_area, int(scale), int(gray_levels), _ptr(out), out.stride(0), col0)
        return 52

    def radial_geometry(self, labels, table: ObjectTable, bin_count: int, maximum_radius: float | None = None) -> torch.Tensor:
        """Ring/wedge code map [F,Y,X] uint8, computed once per (object table, bin_count, maximum_radius).
        maximum_radius=None: scaled rings; a number: unscaled rings of maximum_radius / bin_count pixels + overflow ring."""
        key = bin_count if maximum_radius is None else (bin_count, float(maximum_radius))
        if table._binmaps is None:
            table._binmaps = {}
        if key not in table._binmaps:
            F, Y, X = labels.shape
            binmap = torch.zeros((F, Y, X), dtype=torch.uint8, device=labels.device)
            self._launch("radial_geometry", "aliby_radial_geometry_unscaled", _ptr(labels), F, Y, X, _ptr(table.dev), table.n_obj, table.max_h,
                         table.max_w, int(bin_count), 0.0 if maximum_radius is None else float(maximum_radius), _ptr(binmap))
            table._binmaps[key] = binmap
        return table._binmaps[key]

    def radial_distribution(self, labels, planes, dtype, channel, table: ObjectTable, out, col0, bin_count=4,
                            scaled=True, maximum_radius=100):
        if not scaled and not maximum_radius > 0:
            raise ValueError("radial_distribution(scaled=False) needs maximum_radius > 0")
        binmap = self.radial_geometry(labels, table, bin_count, None if scaled else maximum_radius)
        rings = bin_count if scaled else bin_count + 1
        lab, *rest = self._head(labels, planes, dtype, channel)
        self._launch("radial_distribution", "aliby_features_radial_distribution_rings", lab, _ptr(binmap), *rest, _ptr(table.dev), table.n_obj,
                     int(bin_count), rings, _ptr(out), out.stride(0), col0)
        return 3 * rings

    def granularity(self, labels, planes, dtype, channel, table: ObjectTable, out, col0, subsample_size=0.25,
                    image_sample_size=0.25, element_size=10, granular_spectrum_length=16, image_mask="frame", mask_order=1):
        """cp_measure "granularity" (CellProfiler MeasureGranularity) of `channel` for every object: Granularity_1..L into
        out[:, col0:col0+L].  image_mask: "frame" (CellProfiler's default: no image mask) or "objects" (labels > 0, sampled
        with spline order `mask_order`; only the bilinear order 1 is built).  PARITY UNPINNED — oracle/granularity_restated.py."""
        if image_mask not in ("frame", "objects"):
            raise ValueError(f"image_mask must be 'frame' or 'objects', got {image_mask!r}")
        if image_mask == "objects" and int(mask_order) != 1:
            raise NotImplementedError("granularity(image_mask='objects') is built for mask_order=1 (bilinear) only")
        F, Cn, Y, X = planes.shape
        L = int(granular_spectrum_length)
        need = int(self.lib.aliby_granularity_workspace_bytes(F, Y, X, table.n_obj, float(subsample_size), float(image_sample_size)))
        work = torch.empty((need + 7) // 8, dtype=torch.float64, device=labels.device)
        self._launch("granularity", "aliby_features_granularity", *self._head(labels, planes, dtype, channel), _ptr(table.dev), table.n_obj,
                     float(subsample_size), float(image_sample_size), int(element_size), L, 1 if image_mask == "objects" else 0,
                     _ptr(work), work.numel() * 8, _ptr(out), self._row_stride(out, table.n_obj, col0, L), col0)
        return L

    CELL_COLUMNS = ("area", "centroid_x", "centroid_y", "conical_volume", "eccentricity", "spherical_volume", "volume",
                    "min_ax", "maj_ax", "mean", "median", "std", "total", "total_squared", "max2p5pc", "max5px_median",
                    "moment_of_inertia")

    def cell_metrics(self, labels, planes, dtype, channel, table: ObjectTable) -> torch.Tensor:
        """[n_obj, 17] block of the reference's cell.py metrics (planes may be None: mask-only columns)."""
        out = self.new_output(table.n_obj, 17)
        self._launch("cell_metrics", "aliby_features_cell", *self._head(labels, planes, dtype, channel), _ptr(table.dev), table.n_obj,
                     table.max_h, table.max_w, table.max_area, _ptr(out), self._row_stride(out, table.n_obj, 0, 17), 0)
        return out

    def nuc_est_conv(self, labels, planes, dtype, channel, table: ObjectTable, out, col0, alpha=0.95, object_radius_estimation=0.085,
                     gaussian_sigma=None, median=None):
        """Column col0 of out [n_obj, .]: nuc_est_conv of the reference (custom/localisation.py:75-120) for `channel` of planes
        [F,C,Y,X].  alpha / object_radius_estimation None: the defaults, as there; gaussian_sigma None: derived per object.
        `median`: the objects' medians, float64 [n_obj] on the device (column `median` of cell_metrics, which is where they are
        taken from when not given)."""
        alpha = 0.95 if alpha is None else float(alpha)
        ore = 0.085 if object_radius_estimation is None else float(object_radius_estimation)
        if gaussian_sigma is not None and not (float(gaussian_sigma) > 0.0 and np.isfinite(float(gaussian_sigma))):
            raise ValueError(f"gaussian_sigma must be positive and finite, got {gaussian_sigma!r} (the reference divides by it)")
        if median is None:
            median = self.cell_metrics(labels, planes, dtype, channel, table)[:, self.CELL_COLUMNS.index("median")]
        median = median.contiguous()
        if median.dtype != torch.float64 or median.numel() < table.n_obj:
            raise ValueError("median must hold one float64 per object")
        self._launch("nuc_est_conv", "aliby_features_nuc_est_conv", *self._head(labels, planes, dtype, channel), _ptr(table.dev), table.n_obj,
                     table.max_h, table.max_w, table.max_area, _ptr(median), alpha, ore, 0.0 if gaussian_sigma is None else float(gaussian_sigma),
                     _ptr(out), self._row_stride(out, table.n_obj, col0, 1), col0)
        return 1

    def nuc_conv_3d(self, labels, stack, dtype, channel, table: ObjectTable, out, col0, pixel_size=0.23, z_spacing=0.6):
        """Column col0 of out [n_obj, .]: nuc_conv_3d of the reference (custom/localisation.py:123-140) for `channel` of the
        un-reduced stack [F,C,Z,Y,X]; the objects' 2-D masks are repeated on every plane.  The median and the non-zero count are
        found in the kernel."""
        if stack.ndim != 5:
            raise ValueError(f"stack must be [F,C,Z,Y,X], got shape {tuple(stack.shape)}")
        F, Cn, Z, Y, X = stack.shape
        if tuple(labels.shape) != (F, Y, X):
            raise ValueError(f"labels {tuple(labels.shape)} do not match the stack's [F,Y,X] = {(F, Y, X)}")
        self._launch("nuc_conv_3d", "aliby_features_nuc_conv_3d", _ptr(labels), _ptr(stack), _kdt(dtype), F, Cn, Z, Y, X, int(channel),
                     _ptr(table.dev), table.n_obj, table.max_h, table.max_w, table.max_area, float(pixel_size), float(z_spacing), _ptr(out),
                     self._row_stride(out, table.n_obj, col0, 1), col0)
        return 1

    def cell_ratio(self, labels, planes, dtype, ch0, ch1, table: ObjectTable) -> torch.Tensor:
        """[n_obj] float64: cell.ratio of the reference (cell.py:268-279) for the channel pair (ch0, ch1) of planes [F,C,Y,X]."""
        out = torch.full((max(table.n_obj, 1),), float("nan"), dtype=torch.float64, device=labels.device)
        self._launch("cell_metrics", "aliby_features_cell_ratio", *self._head(labels, planes, dtype, ch0), int(ch1), _ptr(table.dev),
                     table.n_obj, table.max_area, _ptr(out))
        return out[: table.n_obj]

    def trap_background(self, labels, planes, dtype, channel) -> torch.Tensor:
        """[F, 2] float64: (trap.imBackground, trap.background_max5) of every tile (trap.py:6-43): median / mean of the five
        largest of the pixels of `channel` that lie under no mask."""
        out = torch.empty((planes.shape[0], 2), dtype=torch.float64, device=labels.device)
        self._launch("trap_background", "aliby_features_trap_background", *self._head(labels, planes, dtype, channel), _ptr(out))
        return out

    def rank_planes(self, labels, planes, dtype, table: ObjectTable, channels):
        """uint32 [F,C,Y,X] dense ranks + int32 [n_obj,C] maxima for `channels`, cached on the table per plane tensor."""
        F, Cn, Y, X = planes.shape
        key = ("ranks", planes.data_ptr())
        if table._ranks is None:
            table._ranks = {}
        if key not in table._ranks:
            table._ranks[key] = dict(ranks=torch.empty((F, Cn, Y, X), dtype=torch.int32, device=planes.device),
                                     rmax=torch.zeros((max(table.n_obj, 1), Cn), dtype=torch.int32, device=planes.device), done=set())
        e = table._ranks[key]
        for ch in channels:
            if ch in e["done"]:
                continue
            self._launch("ranks", "aliby_object_ranks", *self._head(labels, planes, dtype, ch), _ptr(table.dev), table.n_obj, table.max_area,
                         _ptr(e["ranks"]), _ptr(e["rmax"]))
            e["done"].add(ch)
        return e["ranks"], e["rmax"]

    @staticmethod
    def _coloc_columns(cols: dict) -> tuple:
        """cols of `coloc` -> the columns of (pearson, manders_fold, rwc, costes) as C takes them: -1 for a metric that is not asked for."""
        return tuple(-1 if cols.get(k) is None else int(cols[k]) for k in ("pearson", "manders_fold", "rwc", "costes"))

    def coloc_pairs(self, labels, planes, dtype, pairs, table: ObjectTable, out, thr=15.0, scale_max=255.0) -> bool:
        """All channel pairs in one launch (aliby_features_coloc_pairs).  pairs = [((ch0, ch1), cols), ...] with cols as in
        `coloc`.  False (nothing launched) when the objects' pixel lists do not fit the kernel's LDS budget or there are more
        pairs / channels than one launch takes: the caller then goes pair by pair."""
        chans = sorted({c for (pair, _) in pairs for c in pair})
        any_rwc = any(cols.get("rwc") is not None for _, cols in pairs)
        cap = 64
        while cap < table.max_area:
            cap <<= 1
        if len(pairs) > 28 or len(chans) > 8 or len(chans) * cap * 4 * (2 if any_rwc else 1) > 144 * 1024:
            return False
        ranks = rmax = None
        if any_rwc:
            ranks, rmax = self.rank_planes(labels, planes, dtype, table, tuple(chans))
        spec = np.asarray([[ch0, ch1, *self._coloc_columns(cols)] for (ch0, ch1), cols in pairs], dtype=np.int32)
        self._launch("coloc", "aliby_features_coloc_pairs", *self._head(labels, planes, dtype, 0)[:7], spec.ctypes.data, len(pairs),
                     _ptr(table.dev), table.n_obj, table.max_area, _ptr(out), out.stride(0), float(thr), float(scale_max), _ptr(ranks), _ptr(rmax))
        return True

    def coloc(self, labels, planes, dtype, ch0, ch1, table: ObjectTable, out, cols, thr=15.0, scale_max=255.0):
        """cols = dict(pearson=col|None, manders_fold=..., rwc=..., costes=...)."""
        ranks = rmax = None
        if cols.get("rwc") is not None:
            ranks, rmax = self.rank_planes(labels, planes, dtype, table, (ch0, ch1))
        self._launch("coloc", "aliby_features_coloc", *self._head(labels, planes, dtype, ch0), int(ch1), _ptr(table.dev), table.n_obj,
                     table.max_area, _ptr(out), out.stride(0), *self._coloc_columns(cols), float(thr), float(scale_max), _ptr(ranks), _ptr(rmax))

