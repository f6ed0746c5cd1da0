"""The chunk loop of the per-item evaluations (validation.py, global_eval.py with universal_perturbation.validation, patch_eval.py):
up to `chunk` consecutive items with equal keys are stacked, per chunk a subclass runs its prepare launch, ONE forward and ONE metrics
launch (the scheme of csrc/ufr_common.h) and keeps the result rows on the device, and the host reads them once, at the end.  Next to
the class: what its callers repeat (the pair check, the freeze) and the stage times the tools/bench_* scripts print."""
from __future__ import annotations

import contextlib

import torch

from . import _lib as L


class StageEvents:
    """`events`: None, or the entry's `_debug_events` list; `_mark(stage)` then records a device event at the END of `stage`."""
    events = None

    def _mark(self, stage):
        if self.events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.events.append((stage, ev))


def recorded_events(entry, run):
    """The events of one `run()` with a list on `entry._debug_events` (tools/bench_*), synchronised."""
    entry._debug_events = events = []
    try:
        run()
    finally:
        entry._debug_events = None
    torch.cuda.synchronize()
    return events


def stage_ms(events, stages):
    """{stage: device milliseconds, summed over the chunks ("start" opens one)} of such a list."""
    acc = {s: 0.0 for s in stages}
    for (_, e0), (stage, e1) in zip(events, events[1:]):
        if stage != "start":
            acc[stage] += e0.elapsed_time(e1)
    return acc


def check_pair(first, second, message):
    """Both frames (or both noises) of a batch-1 item: [1,3,H,W] and of one shape, or ValueError(message)."""
    if first.dim() != 4 or first.shape[0] != 1 or first.shape[1] != 3 or second.shape != first.shape:
        raise ValueError(message)


def freeze(net):
    """What every evaluation does before its first forward (`patch_attack.release(net)` gives the flags back)."""
    L.freeze_parameters(net)
    net.eval()


class ChunkedEval(StageEvents):
    """Items waiting for their chunk and the result rows on the device.  A subclass supplies `run_chunk(items)`: the items
    `(key, first tensor, ...)` of one chunk -> its result tensor [K, cols], or a tuple of such."""

    def __init__(self, chunk):
        if int(chunk) < 1:
            raise ValueError("chunk must be positive")
        self.chunk = int(chunk)
        self.waiting, self.rows, self.ws = [], [], None
        self.frozen = False

    def add(self, key, *item):
        """A chunk holds consecutive items of one key, `chunk` at most."""
        if self.waiting and (self.waiting[0][0] != key or len(self.waiting) == self.chunk):
            self.flush()
        self.waiting.append((key,) + item)

    def flush(self):
        """Runs the waiting items as one chunk, on the device of their first tensor."""
        if not self.waiting:
            return
        items, self.waiting = self.waiting, []
        dev = getattr(items[0][1], "device", None)
        guard = torch.cuda.device(dev) if dev is not None and dev.type == "cuda" else contextlib.nullcontext()
        with guard, torch.no_grad():
            out = self.run_chunk(items)
        self.rows.append(out if isinstance(out, tuple) else (out,))

    def run_chunk(self, items):
        raise NotImplementedError

    def read(self):
        """The one host synchronisation: the tail, then per result tensor of `run_chunk` all rows in arrival order (numpy); [] if none."""
        self.flush()
        return [torch.cat(col).cpu().numpy() for col in zip(*self.rows)]

    def freeze_once(self, net):
        """`freeze(net)` at the first item: a loader without items leaves the network as it was."""
        if not self.frozen:
            freeze(net)
            self.frozen = True

    @staticmethod
    def stack_f32(tensors, dev):
        """Batch-1 tensors -> one contiguous float32 stack on the chunk's device."""
        return torch.cat([t.detach().to(device=dev, dtype=torch.float32) for t in tensors]).contiguous()

    def workspace(self, doubles, dev):
        """The float64 workspace of the metrics launch, reallocated when a chunk needs more or another device."""
        if self.ws is None or self.ws.device != dev or self.ws.numel() < doubles:
            self.ws = torch.zeros(doubles, dtype=torch.float64, device=dev)
        return self.ws

    @staticmethod
    def checked_flow(flow, pairs, H, W, same_size=False):
        """The network's answer for `pairs` stacked pairs of HxW frames: [pairs,2,h,w] (h x w = H x W with `same_size`)."""
        bad = tuple(flow.shape) != (pairs, 2, H, W) if same_size else flow.dim() != 4 or flow.shape[0] != pairs or flow.shape[1] != 2
        if bad:
            raise RuntimeError(f"the network returned a flow of shape {tuple(flow.shape)} for {pairs} pairs of {H}x{W} frames")
        return flow
