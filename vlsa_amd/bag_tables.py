"""The tables the multi-bag kernels read, built in ONE place: descriptor rows (pointer, N_i, row stride -- ``vlsa_bag_desc``), bag
validation, the pinned upload ring, and ``ChunkTables`` -- descriptor, row offsets and tile_start of a chunk of <= 64 bags, packed on
the host into one upload or derived on the device from a descriptor that is already up.  A wrong table is a device fault, so every
batched route of ``functional.py`` takes its tables from here."""
from __future__ import annotations

import ctypes
import threading
from typing import Optional

import numpy as np
import torch

from . import _native as nat
from ._native import VlsaNativeError

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current HIP stream of the current device as a C pointer.  The raw accessors (what torch.cuda.current_stream() wraps) save
    ~7 us of Python object construction per call -- this runs several times per bag in the bag-by-bag loops."""
    if _raw_stream is not None and _cur_device is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dt(X):
    return nat.DT_F32 if X.dtype == torch.float32 else nat.DT_BF16


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise VlsaNativeError(
                "vlsa_amd runs on MI355X only: got a CPU tensor (there is no CPU fallback; the CPU oracle under "
                "oracle/ is test infrastructure)")


_BAG_DTYPES = (torch.bfloat16, torch.float32)


def _bag2d(X: torch.Tensor) -> torch.Tensor:
    """[1,N,D] or [N,D] -> [N,D] view with unit inner stride and 16-byte aligned rows (copy only if needed)."""
    # the common case first (a list of 64 slide-sized bags pays this per bag, and the launch itself is ~0.6 us per bag): a contiguous
    # [N, D] bf16 / fp32 tensor whose rows are a multiple of 16 bytes, at a 16-byte aligned address
    if (X.dim() == 2 and X.dtype in _BAG_DTYPES and X.is_contiguous() and (X.shape[1] * X.element_size()) % 16 == 0
            and X.data_ptr() % 16 == 0):
        return X
    if X.dim() == 3:
        if X.shape[0] != 1:
            raise AssertionError("X.shape[0] must be 1 (one bag per call; model/deepmil.py:175)")
        X = X[0]
    if X.dim() != 2:
        raise ValueError(f"expected a [N, D] or [1, N, D] bag, got {tuple(X.shape)}")
    if X.dtype not in (torch.float32, torch.bfloat16):
        X = X.float()
    esz = X.element_size()
    if X.shape[0] > 0 and (X.stride(1) != 1 or (X.stride(0) * esz) % 16 != 0 or X.data_ptr() % 16 != 0
                           or X.stride(0) < X.shape[1]):
        X = X.contiguous()
    return X


def bag_rows(bags, D=None, empty_stride=None) -> np.ndarray:
    """int64 [B, 3] descriptor rows (data_ptr, N_i, row stride in elements) of [N_i, D] tensors: THE place that writes such a row.
    An empty bag's tensor may carry any stride: where the kernel checks ``stride >= D`` before it looks at N (the streaming batch
    kernels: ``_BagTable``, ``VlfanBatchPlan.set_bags``) the caller gives D (or another ``empty_stride``) for such a row; else its own."""
    es = D if empty_stride is None else empty_stride
    if es is None:
        rows = [(x.data_ptr(), x.shape[0], x.stride(0)) for x in bags]
    else:
        rows = [(x.data_ptr(), x.shape[0], x.stride(0) if x.shape[0] > 0 else es) for x in bags]
    return np.asarray(rows, dtype=np.int64).reshape(len(rows), 3)


def _fits(x, D: int, dtype, device, non_empty: bool) -> bool:
    """THE per-bag condition of the batched routes: [N, D] or [1, N, D], the dtype and device of the first bag (whose dtype the caller
    has found among bf16 / fp32), N >= 1 where asked.  (One ``shape`` per bag: a list of 64 bags pays this per bag.)"""
    s = x.shape
    return ((len(s) == 2 or (len(s) == 3 and s[0] == 1)) and s[-1] == D and x.dtype == dtype and x.device == device
            and (s[-2] >= 1 or not non_empty))


def checked_bags(bags, D: int, message: str, non_empty: bool = False, no_grad: Optional[str] = None) -> list:
    """Every bag on the GPU and through ``_bag2d``; all of width D, one dtype (bf16 or fp32) and one device -- else
    ``VlsaNativeError(message)``.  non_empty: N_i >= 1 as well.  no_grad: the message for a bag that requires grad while grad is
    enabled (None: not checked).  Returns the [N_i, D] views."""
    keep = []
    for x in bags:
        _need_gpu(x)
        x = _bag2d(x)                       # (bf16 or fp32 behind it: other dtypes come out as fp32 copies)
        first = keep[0] if keep else x
        if not _fits(x, D, first.dtype, first.device, non_empty):
            raise VlsaNativeError(message)
        if no_grad is not None and torch.is_grad_enabled() and x.requires_grad:
            raise VlsaNativeError(no_grad)
        keep.append(x)
    return keep


def is_bag_set(bags) -> bool:
    """a ``functional.BagSet`` (which imports this module): checked bags with their ``sizes`` and kept ``chunk`` sub-sets"""
    return hasattr(bags, "sizes") and hasattr(bags, "chunk")


def uniform_bags(bags, D: int = 512) -> bool:
    """``checked_bags(bags, D, ..., non_empty=True)`` without raising and without converting: whether the batched routes take these
    bags as they are -- a ``BagSet`` of width D (checked when it was built), or a non-empty sequence of device tensors [N >= 1, D]
    or [1, N, D] of one dtype (bf16 or fp32) on one device.  A gradient of the bags is the caller's question."""
    if is_bag_set(bags):
        return bags.D == D
    if len(bags) == 0:
        return False
    dtype, device = bags[0].dtype, bags[0].device
    return dtype in _BAG_DTYPES and all(x.is_cuda and _fits(x, D, dtype, device, True) for x in bags)


def bag_chunks(bags, n: int = 64, max_rows: Optional[int] = None):
    """The chunks of <= n bags a batched route launches on, in order.  A ``BagSet`` hands out ``bags.chunk(i, n)`` -- itself when it
    fits, else its kept sub-sets, each with its device-side table; a list (or the ``ProjectedBags`` of one chunk) goes out as it is
    when it fits and as slices otherwise.  max_rows: a chunk also closes before the bag that would take it past ``max_rows`` rows, and
    a bigger bag travels alone."""
    B, is_set = len(bags), is_bag_set(bags)
    if max_rows is None:
        if is_set:
            for i in range(0, B, n):
                yield bags.chunk(i, n)
        elif 0 < B <= n:
            yield bags
        else:
            for i in range(0, B, n):
                yield bags[i:i + n]
        return
    sizes = bags.sizes if is_set else [int(x.shape[0]) for x in bags]
    i = 0
    while i < B:
        j, rows = i + 1, sizes[i]
        while j < B and j - i < n and rows + sizes[j] <= max_rows:
            rows += sizes[j]
            j += 1
        yield bags.chunk(i, j - i) if is_set else (bags if j - i == B else bags[i:j])
        i = j


def cat(parts):
    """the results of a route's chunks as one tensor: the only one as it is"""
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def merge_strides(G: int, P: int, D: int, out=None):
    """the nine element strides ``vlsa_vlfan_merge_batch_strided`` takes for (pm, pl, pacc): between a bag's G partials, between bags,
    and between the bags' outputs (m2, l, out) -- ``out``: those three; default: dense [B, 16], [B, 16], [B, P, D]"""
    S = nat.P_STRIDE
    return (ctypes.c_int64 * 9)(S, S, P * D, G * S, G * S, G * P * D, *(out or (S, S, P * D)))


# ---- upload ---------------------------------------------------------------------------------------------------------------------
class _PinnedRing:
    """Small ring of pinned int64 staging buffers for the descriptor tables of the multi-bag kernels: the upload is an ASYNC copy
    on the current stream (a pageable `.to(device)` blocks the host for tens of microseconds per call); a slot is reused only after
    the copy that read it has completed (event)."""

    def __init__(self, slots: int = 8, words: int = 1024):
        self.slots, self.words, self.bufs, self.events, self.i = slots, words, None, None, 0

    def stage(self, host_np, device, route: str):
        n = int(host_np.shape[0])
        if not torch.cuda.is_available():
            return torch.from_numpy(np.ascontiguousarray(host_np)).to(device)
        no_capture(route)
        if n > self.words:
            return torch.from_numpy(np.ascontiguousarray(host_np)).to(device)
        if self.bufs is None:
            self.bufs = [torch.empty(self.words, dtype=torch.int64).pin_memory() for _ in range(self.slots)]
            self.events = [None] * self.slots
        k = self.i % self.slots
        self.i += 1
        if self.events[k] is not None:
            self.events[k].synchronize()
        self.bufs[k].numpy()[:n] = host_np
        dev = self.bufs[k][:n].to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self.events[k] = ev
        return dev


_TABLE_RING = {}     # per host thread (autograd runs backward functions on its own thread)


def no_capture(route: str):
    """A table staged from the host cannot go up inside a graph capture (a replay would copy whatever the staging buffer then holds):
    the routes that capture derive their tables on the device from a ``BagSet``'s descriptor, uploaded before the capture."""
    if torch.cuda.is_current_stream_capturing():
        raise VlsaNativeError(f"{route}: its table is staged from the host, which a graph capture cannot hold -- capture over a "
                              "BagSet whose descriptor table is up (BagSet.desc()); the other tables are then derived on the device")


def _stage_table(host_np, device, route: str) -> torch.Tensor:
    """int64 table -> device through a ring of pinned staging buffers (async; a pageable ``.to(device)`` blocks the host for ~60 us
    per call -- four such copies were 0.25 ms of a 2.1 ms optimizer step).  THE upload route of the batched paths; ``route`` names
    the caller in the error raised under a graph capture."""
    ring = _TABLE_RING.setdefault(threading.get_ident(), _PinnedRing())
    return ring.stage(host_np.reshape(-1), device, route).view(host_np.shape)


# ---- the tables of one chunk ----------------------------------------------------------------------------------------------------
def pack_tables(rows: np.ndarray, tile_rows: int, rows2: Optional[np.ndarray] = None):
    """The host image of ONE upload: descriptor rows [B, 3] | a second descriptor table [B, 3] (``rows2``: gradient or output rows) |
    row offsets [B] (int64) | tile_start [B + 1] (int32, tiles of ``tile_rows`` rows, padded to whole int64 words).
    Returns (int64 words, row offsets [B + 1], n_tiles)."""
    B = len(rows)
    o = 3 * B if rows2 is None else 6 * B
    host = np.zeros(o + B + (B + 2) // 2, dtype=np.int64)
    host[:3 * B] = rows.reshape(-1)
    if rows2 is not None:
        host[3 * B:o] = rows2.reshape(-1)
    offs = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(rows[:, 1], out=offs[1:])
    host[o:o + B] = offs[:B]
    ts = host[o + B:].view(np.int32)
    np.cumsum((rows[:, 1] + (tile_rows - 1)) // tile_rows, out=ts[1:B + 1])
    return host, offs, int(ts[B])


class ChunkTables:
    """What the kernels over a chunk of <= 64 bags read: ``desc`` [B, 3] (``bag_rows``), ``desc2`` (a second such table, or None),
    ``row_off`` [B] (int64: first row of each bag among the chunk's rows laid back to back) and ``tile_start(tile_rows)`` -- device
    tensors -- with the host's view of the same: ``sizes``, ``offs`` [B + 1], ``total``, ``dt``.  A launch takes the addresses
    (``p_desc``, ``p_desc2``, ``p_row_off``, ``p_tile_start(tile_rows)``): of a packed upload they are known without cutting a
    tensor view per table, which the bag-by-bag training loop cannot afford.  ``keep`` is the device memory behind them: whoever
    launches a kernel on them holds this object until the result is dropped."""

    def __init__(self, sizes, dt: int, keep, p_desc: int, p_row_off: int, p_desc2: Optional[int] = None, offs=None):
        self.B, self.sizes, self.dt, self.keep = len(sizes), sizes, dt, keep
        self.p_desc, self.p_desc2, self.p_row_off = p_desc, p_desc2, p_row_off
        if offs is None:
            offs = np.zeros(self.B + 1, dtype=np.int64)
            np.cumsum(sizes, out=offs[1:])
        self.offs, self.total = offs, int(offs[-1])
        self._ts, self._views = {}, None            # tile_rows -> [address, n_tiles, tensor or None]; (desc, desc2, row_off)

    @classmethod
    def from_host(cls, rows: np.ndarray, dt: int, tile_rows: int, device, route: str, rows2=None) -> "ChunkTables":
        """everything in ONE staged upload (``pack_tables``); tile_start for ``tile_rows`` comes with it"""
        host, offs, n_tiles = pack_tables(rows, tile_rows, rows2)
        return cls._of_words(_stage_table(host, device, route), rows[:, 1].tolist(), dt, tile_rows, n_tiles, rows2 is not None, offs)

    @classmethod
    def from_one_bag(cls, x: torch.Tensor, tile_rows: int, extra: Optional[torch.Tensor] = None) -> "ChunkTables":
        """one non-empty bag (the bag-by-bag training loop): the same words written ON the device from by-value arguments -- one
        launch instead of numpy bookkeeping + a pinned staging copy + an event per call; 64 bytes, no state shared between calls"""
        buf, n = torch.empty(8, dtype=torch.int64, device=x.device), x.shape[0]
        n_tiles = nat.load().vlsa_fill_one_bag_tables(_p(buf), _p(x), n, x.stride(0), _p(extra),
                                                      0 if extra is None else extra.stride(0), int(tile_rows), _stream())
        if n_tiles < 0:
            nat.check(n_tiles, "vlsa_fill_one_bag_tables")
        return cls._of_words(buf, [n], _dt(x), tile_rows, int(n_tiles), extra is not None, (0, n))

    @classmethod
    def _of_words(cls, words, sizes, dt, tile_rows, n_tiles, two, offs):
        B, base = len(sizes), words.data_ptr()
        o = 6 * B if two else 3 * B
        t = cls(sizes, dt, words, base, base + 8 * o, base + 24 * B if two else None, offs)
        t._ts[tile_rows] = [base + 8 * (o + B), n_tiles, None]
        return t

    @classmethod
    def from_device(cls, desc: torch.Tensor, sizes, dt: int) -> "ChunkTables":
        """from a descriptor that is already up, by in-stream ops: nothing is staged, so this also runs inside a graph capture"""
        n = desc[:, 1]
        row_off = (torch.cumsum(n, 0) - n).contiguous()
        t = cls(sizes, dt, (desc, row_off), desc.data_ptr(), row_off.data_ptr())
        t._views = (desc, None, row_off)
        return t

    @classmethod
    def of_list(cls, bags, tile_rows: int, route: str, extra=None) -> "ChunkTables":
        """a plain list of device bags (``extra``: one gradient / output tensor per bag for the second table)"""
        if len(bags) == 1 and bags[0].shape[0] > 0:
            return cls.from_one_bag(bags[0], tile_rows, None if extra is None else extra[0])
        return cls.from_host(bag_rows(bags), _dt(bags[0]), tile_rows, bags[0].device, route, None if extra is None else bag_rows(extra))

    def _tensors(self):
        """(desc, desc2, row_off) as tensors; of a packed upload: views of its words, cut on first use"""
        if self._views is None:
            B, w = self.B, self.keep
            o = (self.p_row_off - self.p_desc) // 8
            self._views = (w[:3 * B].view(B, 3), None if self.p_desc2 is None else w[3 * B:6 * B].view(B, 3), w[o:o + B])
        return self._views

    desc = property(lambda self: self._tensors()[0])
    desc2 = property(lambda self: self._tensors()[1])
    row_off = property(lambda self: self._tensors()[2])

    def p_tile_start(self, tile_rows: int):
        """(address of tile_start, n_tiles): what a launch takes"""
        if tile_rows not in self._ts:
            self.tile_start(tile_rows)
        return tuple(self._ts[tile_rows][:2])

    def tile_start(self, tile_rows: int):
        """(device int32 [B + 1]: first tile of each bag when every bag is cut into tiles of ``tile_rows`` rows, n_tiles); derived
        from ``desc`` by in-stream ops where the upload did not bring it, and kept per height"""
        t = self._ts.get(tile_rows)
        if t is None:
            n = self.desc[:, 1]
            ts = torch.zeros(self.B + 1, dtype=torch.int32, device=n.device)
            ts[1:] = torch.cumsum(torch.div(n + (tile_rows - 1), tile_rows, rounding_mode="floor"), 0)
            t = self._ts[tile_rows] = [ts.data_ptr(), sum((k + tile_rows - 1) // tile_rows for k in self.sizes), ts]
        elif t[2] is None:       # the upload's own: a view of its words
            t[2] = self.keep[(t[0] - self.p_desc) // 8:].view(torch.int32)[:self.B + 1]
        return t[2], t[1]

    def packed_desc(self, base_ptr: int) -> torch.Tensor:
        """the [B, 3] descriptor of the chunk's rows laid back to back as fp32 [total, 512] at ``base_ptr`` (in-stream ops)"""
        n = self.desc[:, 1]
        return torch.stack([self.row_off * 2048 + base_ptr, n, torch.full_like(n, 512)], 1).contiguous()
