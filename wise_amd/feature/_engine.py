"""What the feature engines (VitEngine, TextEngine, XlmrTextEngine, HtsatEngine, Cnn14Engine) share, each rule once:
the weight blobs' size check, the workspace's growth, graph capture and replay of small token batches, and whole batches
kept in flight on streams of their own.  Host plumbing only: nothing here computes, every kernel is behind the C call the
engine itself makes."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .._streams import concurrent_streams


def device_blobs(counts: Tuple[int, int], packed, device, what: str):
    """packed (bf16 blob, fp32 blob) -> their device copies, once their element counts equal the library's two layout
    `counts`; `what` names the layout in the error."""
    (nb, nf), (wb, pf) = counts, packed
    if wb.numel() != nb or pf.numel() != nf:
        raise RuntimeError(f"{what}: blob size mismatch: packed {wb.numel()}/{pf.numel()}, library expects {nb}/{nf}")
    return wb.to(device), pf.to(device)


def fit_workspace(held: Optional[torch.Tensor], nbytes: int, device, unsupported: Exception,
                  on_grow: Optional[Callable[[], None]] = None) -> torch.Tensor:
    """The one growth rule: `nbytes` is what the library asks for this call (0: a shape it does not support ->
    `unsupported` is raised); `held` is returned as it is unless it is smaller, so a workspace never shrinks.  `on_grow`
    runs before `held` is replaced: whatever still uses the old block, or remembers its address, is dealt with there."""
    if nbytes == 0:
        raise unsupported
    if held is not None and held.numel() >= nbytes:
        return held
    if on_grow is not None:
        on_grow()
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


class Engine:
    """Base of the five: `lib`, `device`, the device copies `wb` / `pf` of the weight blobs and the workspace `_ws` that
    `forward` used last (the `residual` / `tap` methods read it).  The helper objects below hold no reference to their
    engine (it is handed to each call), so an engine and its device memory go when the last name for it goes."""

    _slots = property(lambda self: self._inflight.slots)     # of the engines that keep batches in flight

    def _load(self, device, layout: str, pack: Callable[[], tuple], *cfg):
        """`layout`: the library's wise_*_layout, called with `cfg` in front of the two counts; `pack()` -> the blobs"""
        self.lib = _lib.lib()
        self.device = torch.device(device)
        nb, nf = C.c_int64(), C.c_int64()
        _lib.check(getattr(self.lib, layout)(*cfg, C.byref(nb), C.byref(nf)), layout)
        self.wb, self.pf = device_blobs((nb.value, nf.value), pack(), self.device, layout)
        self._ws = None

    def _fit(self, nbytes: int, unsupported: Exception, on_grow: Optional[Callable[[], None]] = None):
        self._ws = fit_workspace(self._ws, nbytes, self.device, unsupported, on_grow)


class GraphReplay:
    """Small token batches as captured graphs.  One query is 86 - 175 launches of a few microseconds each: launch-bound.
    The C ABI allocates and synchronises nothing, so a forward is capturable: a batch size is captured once into a
    hipGraph on static tokens / output and replayed from then on.  `engine.graph_max_batch` (a plain attribute the
    engine's constructor sets to 4; 0 turns this off) is the largest batch that goes this way.  The engine supplies
    `_launch(tokens, out)`, and `_placeholder(B)`: valid tokens for the warm-up launch."""

    def __init__(self):
        self.table = {}                 # B -> (graph, static tokens, static out)

    def __len__(self):
        return len(self.table)

    def clear(self):
        """captured graphs hold the workspace's address: the engine's `reserve` has them go when it is replaced"""
        self.table.clear()

    def _graph_for(self, e: Engine, B: int):
        hit = self.table.get(B)
        if hit is None:
            tok = e._placeholder(B)
            out = torch.empty(B, e.spec.embed_dim, dtype=torch.float32, device=e.device)
            e._launch(tok, out)  # warm-up outside the capture (first-call kernel attributes)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            try:
                # thread-local capture mode: other threads of the process (e.g. the RCCL watchdog) may call the
                # runtime while this thread captures
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    e._launch(tok, out)
            except RuntimeError:
                e.graph_max_batch = 0   # capture not possible here: keep launching directly (same kernels)
                torch.cuda.synchronize()
                return None
            hit = self.table[B] = (g, tok, out)
        return hit

    def forward(self, e: Engine, t: torch.Tensor) -> torch.Tensor:
        """validated int32 device tokens [B, context] (the workspace already fits them) -> [B, D] fp32"""
        B = t.shape[0]
        if B <= e.graph_max_batch and not torch.cuda.is_current_stream_capturing():
            hit = self._graph_for(e, B)
            if hit is not None:
                g, tok, gout = hit
                tok.copy_(t)
                g.replay()
                return gout.clone()
        out = torch.empty(B, e.spec.embed_dim, dtype=torch.float32, device=e.device)
        e._launch(t, out)
        return out


class _CopyStream:
    """The stream results leave on: SEEN to run beside the slots' own (on the hardware queue of one of them a copy of
    batch i would sit behind batch i + 1's forward), chosen when first asked for.  All a result handle keeps of the
    engine that made it: streams, no workspace and no weights."""

    def __init__(self, device, beside):
        self.device, self.beside, self.stream = device, beside, None

    def get(self) -> "torch.cuda.Stream":
        if self.stream is None:
            self.stream = concurrent_streams(1, self.device, beside=self.beside)[0]
        return self.stream


class PendingEmbeddings:
    """Handle of a batch enqueued by an engine's forward_pipelined."""

    def __init__(self, out: torch.Tensor, done: "torch.cuda.Event", copy: _CopyStream):
        self._out, self._done, self.copy = out, done, copy

    def result(self) -> torch.Tensor:
        """The embeddings [B, D], ordered after the batch on the caller's current stream (no host sync)."""
        torch.cuda.current_stream(self._out.device).wait_event(self._done)
        return self._out


class InFlight:
    """Whole batches in flight: successive `submit`s go round `engine.batches_in_flight` slots (a plain attribute the
    engine's constructor sets to 2, read on every call; at least 1), each slot a stream and a workspace of its own, so the
    GPU always holds that many batches: a batch runs with full-batch GEMM shapes and the other batches' kernels fill its
    LayerNorm / attention phases and tails.  `slots` is the list of {"stream", "ws"} the engine shows as `_slots` (the
    same list object throughout), empty before the first submit."""

    def __init__(self):
        self.slots = []
        self.next = 0
        self.copy = None

    def submit(self, e: Engine, x: torch.Tensor, out_dim: int, need: int, unsupported: Exception, name: str,
               call: Callable[[torch.Tensor, torch.Tensor, torch.Tensor, int], int]) -> PendingEmbeddings:
        """Enqueue the engine's C call `call(x, out, workspace, stream) -> rc` (`name` in its error) on device input `x`,
        which was produced on the caller's current stream and needs `need` workspace bytes; returns at once."""
        depth = max(1, int(e.batches_in_flight))
        if len(self.slots) < depth:
            if self.slots:
                torch.cuda.synchronize(e.device)     # depth raised on a live engine: nothing may still run in the old slots
            # streams SEEN to run side by side (two on one hardware queue: no overlap), all chosen together
            self.slots[:] = [{"stream": st, "ws": None} for st in concurrent_streams(depth, e.device)]
            self.next, self.copy = 0, None
        if self.copy is None:
            self.copy = _CopyStream(e.device, [sl["stream"] for sl in self.slots])
        slot = self.slots[self.next % depth]         # a depth lowered since: the first `depth` slots
        self.next = (self.next + 1) % depth
        stream = slot["stream"]
        # the old workspace may still be in use by this slot's previous forward, and it was allocated on another stream
        # than the one that uses it: wait for that forward before the allocator may hand the block out again
        slot["ws"] = fit_workspace(slot["ws"], need, e.device, unsupported, stream.synchronize)
        stream.wait_stream(torch.cuda.current_stream(e.device))      # the batch was produced on the caller's stream
        out = torch.empty(x.shape[0], out_dim, dtype=torch.float32, device=e.device)
        x.record_stream(stream)
        out.record_stream(stream)
        e.lib.wise_overlap_hint(1)      # this batch runs beside the other slots': GEMM tiles chosen for co-residency
        try:
            rc = call(x, out, slot["ws"], stream.cuda_stream)
        finally:
            e.lib.wise_overlap_hint(0)
        _lib.check(rc, name)
        done = torch.cuda.Event()
        done.record(stream)
        return PendingEmbeddings(out, done, self.copy)


class _AsyncFeatures:
    """Embeddings on their way to the host: copy queued behind the forward on a side stream, `.result()` waits for it."""

    def __init__(self, pending: PendingEmbeddings):
        cs = pending.copy.get()
        with torch.cuda.stream(cs):
            out = pending.result()                     # orders the copy stream after the forward
            self._host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
            self._host.copy_(out, non_blocking=True)
            out.record_stream(cs)
            self._done = torch.cuda.Event()
            self._done.record(cs)

    def result(self) -> np.ndarray:
        self._done.synchronize()
        return self._host.numpy()
