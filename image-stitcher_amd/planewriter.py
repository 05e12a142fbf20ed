"""The slot ring behind the streaming writers (omezarr.PlaneStreamWriter, ometiff.PyramidTiffWriter)."""
from typing import Sequence

import numpy as np


class SlotRingWriter:
    """Streams fused planes from the device to a target that a subclass writes.

    Two slots, each = a device canvas of ``batch`` planes, device buffers for its pyramid levels and
    pinned host mirrors of all of them.  ``acquire(m)`` hands out the slot's canvas (waiting until the
    slot's previous contents are on disk); the caller fuses into it on the current stream and calls
    ``submit(coords)``, which enqueues the pyramid kernels (and, for a writer that encodes on the device, the encoder of every
    level) behind the fusion and the D2H copies on a separate copy stream behind those, and returns at once; a dispatcher
    thread waits for the copies and hands the slot to the subclass.  So batch k is copied out, compressed and
    written while batch k+1 is read, copied in and fused.

    A subclass sets its own attributes, calls ``_init_ring`` and then ``_thread.start()``, and supplies:
    ``_make_encoder(lv, yx, device)`` (the native.*Buffers of a level), ``_encode(planes, enc)``, ``_overflow_message()``,
    ``_target()`` (what travels with a queued batch: where it goes), ``_write_streams(slot, coords, target, totals)`` /
    ``_write_planes(slot, coords, target)`` (what is done with a slot whose packed streams / raw planes are on the host) and
    ``_shutdown(joined)`` (what ``close`` ends besides the thread).  One that queues ``(None, None, None, target)`` items --
    "this target is complete" -- also supplies ``_finish(target)`` and names its last such item in ``_last_item()``.
    """
    thread_name = 'plane-writer'

    def _init_ring(self, shapes: Sequence[tuple], dtype, *, batch: int, device, slots: int, buffers, canvas_arena,
                   pyramid_method: str, encoded: bool) -> None:
        import queue
        import threading
        import torch
        from . import native, omezarr
        self.batch = int(batch)
        # 'mean': all levels of a slot from one read of its canvas (sq_pyramid_mean) instead of one launch per level
        self.pyramid_method = omezarr.check_pyramid_method(pyramid_method)
        self.bytes_written = 0
        # optional target of the value counts of level 0: a device int64 [C, bins] tensor; submit() adds the planes it is handed
        # to row c of it (sq_histogram_planes).  None: nothing is launched.  Callers set it per target (``retarget`` keeps it).
        self.histogram = None
        # optional composite.CompositeTarget: submit() hands it the planes (and this writer's row offset) before the slot is
        # released, so that it can reduce its source planes where they are final.  None: nothing is launched.
        self.composite = None
        tdtype = native.torch_dtype_of(np.dtype(dtype).type)
        yx = [tuple(int(v) for v in s[3:]) for s in shapes]
        # ``buffers``: the (device, pinned host) slot buffers of an earlier writer of the same geometry --
        # page-locking host memory costs more than a small region's whole fusion, so callers that write
        # many regions (one per well and timepoint) hand them on
        if buffers is None:
            # level 0 = the fusion canvas: dense rows, planes on 128-byte lines (native.empty_canvas)
            # (canvas_arena: a native.DeviceArena to carve the level-0 canvases from -- memory mapped over all memory classes of
            #  the card, where the fusion kernel writes fastest; the slot tensors keep it alive)
            dev = [[native.empty_canvas(self.batch, s[0], s[1], tdtype, device, arena=canvas_arena) if lv == 0 else
                    torch.empty((self.batch,) + s, dtype=tdtype, device=device) for lv, s in enumerate(yx)] for _ in range(slots)]
            if encoded:
                # chunks / tiles are encoded on the device: the host mirrors hold packed STREAMS, not planes
                enc = [[self._make_encoder(lv, s, device) for lv, s in enumerate(yx)] for _ in range(slots)]
                host = [[(torch.empty(e.bound, dtype=torch.uint8, pin_memory=True),
                          torch.empty(e.n_chunks + 1, dtype=torch.int64, pin_memory=True),
                          torch.empty(1, dtype=torch.int32, pin_memory=True)) for e in slot_enc] for slot_enc in enc]
                buffers = (dev, host, enc)
            else:
                buffers = (dev, [[torch.empty((self.batch,) + s, dtype=tdtype, pin_memory=True) for s in yx] for _ in range(slots)])
        self.buffers = buffers
        if encoded != (len(buffers) == 3):
            raise ValueError("buffers do not match this writer's compression")
        self._dev, self._host = buffers[0], buffers[1]
        self._enc = buffers[2] if encoded else None
        if len(self._dev) != slots or [tuple(t.shape) for t in self._dev[0]] != [(self.batch,) + s for s in yx] \
                or self._dev[0][0].dtype != tdtype:
            raise ValueError("buffers do not match this writer's geometry")
        # D2H copies run on their own stream: the link is full duplex, so batch k leaves the device while
        # batch k+1's tiles arrive and are fused on the caller's stream
        self._copy_stream = torch.cuda.Stream(device=device)
        # ... and the writer thread fetches a slot's packed streams on a stream of ITS own: on _copy_stream they would
        # queue behind the wait for the NEXT slot's fusion (submit() parks that wait there) and the disk write-out the
        # two slots are meant to overlap would serialise
        self._frame_stream = torch.cuda.Stream(device=device)
        self._free = [threading.Event() for _ in range(slots)]
        for e in self._free:
            e.set()
        self._slot, self._m, self._error = -1, 0, None
        self._queue: "queue.Queue" = queue.Queue()
        self._thread = threading.Thread(target=self._dispatch, name=self.thread_name, daemon=True)

    def _dispatch(self):
        while True:
            item = self._queue.get()
            if item is None:
                return
            slot, coords, event, target = item
            try:
                if slot is None:          # the target is complete behind everything submitted to it
                    self._finish(target)
                    continue
                event.synchronize()
                if self._enc is not None:
                    self._write_streams(slot, coords, target, self._fetch_streams(slot, len(coords)))
                else:
                    self._write_planes(slot, coords, target)
            except BaseException as exc:   # surfaced by the next acquire() / drain() / close()
                self._error = exc
            finally:
                if slot is not None:
                    self._free[slot].set()

    def _fetch_streams(self, slot: int, m: int) -> list:
        """The offsets of this slot are on the host; fetch exactly the packed streams of its ``m`` planes (only compressed bytes
        cross PCIe) into the slot's page-locked buffers -> their size per level."""
        import torch
        done = torch.cuda.Event()
        totals = []
        with torch.cuda.stream(self._frame_stream):     # the encoder has finished: _dispatch waited for the slot's event
            for enc, (frames, offsets, status) in zip(self._enc[slot], self._host[slot]):
                if int(status[0]):
                    raise RuntimeError(self._overflow_message())
                total = int(offsets[m * (enc.n_chunks // self.batch)])
                totals.append(total)
                if total:
                    frames[:total].copy_(enc.out[:total], non_blocking=True)
            done.record()
        done.synchronize()
        return totals

    def _check(self):
        if self._error is not None:
            err, self._error = self._error, None
            raise err

    def acquire(self, m: int):
        """Device canvas [m, Hc, Wc] of the next slot (contents undefined)."""
        if not 0 < m <= self.batch:
            raise ValueError(f"a slot holds 1..{self.batch} planes, asked for {m}")
        self._slot = (self._slot + 1) % len(self._dev)
        self._free[self._slot].wait()
        self._check()
        self._m = m
        return self._dev[self._slot][0][:m]

    def submit(self, coords: Sequence[tuple]) -> None:
        """The canvas handed out by the last ``acquire`` is (being) filled on the current stream."""
        import torch
        from . import native, omezarr
        slot, m = self._slot, self._m
        if len(coords) != m:
            raise ValueError(f"{m} planes acquired, {len(coords)} coordinates given")
        dev = self._dev[slot]
        if self.histogram is not None:      # the m planes handed in, not the padding of a partly filled slot
            native.histogram_planes(dev[0][:m], [c for _, c, _ in coords], hist=self.histogram)
        if self.composite is not None:
            self.composite.add(dev[0][:m], coords, self.row_offset)
        omezarr.device_levels(dev[0][:m], len(dev), out=dev[1:], method=self.pyramid_method)
        if self._enc is not None:      # encode every level behind the pyramid, on the caller's stream
            for lv, enc in enumerate(self._enc[slot]):
                full = dev[lv]     # the buffers are sized for a full batch: what lies past m is zeroed and costs no bytes
                self._encode(full if m == self.batch else omezarr._pad_planes(full, m), enc)
        fused = torch.cuda.Event()
        fused.record()                                  # fusion + pyramid (+ encoding) of this slot, on the caller's stream
        event = torch.cuda.Event()
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(fused)
            if self._enc is not None:
                for enc, (frames, offsets, status) in zip(self._enc[slot], self._host[slot]):
                    offsets.copy_(enc.offsets, non_blocking=True)
                    status.copy_(enc.status, non_blocking=True)
            else:
                for d, h in zip(dev, self._host[slot]):
                    if d.is_contiguous():
                        h[:m].copy_(d[:m], non_blocking=True)
                    else:                       # padded plane stride: every plane is contiguous, the stack is not
                        for p in range(m):
                            h[p].copy_(d[p], non_blocking=True)
            event.record()
        self._free[slot].clear()
        self._queue.put((slot, list(coords), event, self._target()))

    def drain(self) -> None:
        """Wait until everything submitted so far is written (the writer stays usable)."""
        for e in self._free:
            e.wait()
        self._check()

    def close(self):
        for e in self._free:
            e.wait()
        joined = self._thread.is_alive()
        if joined:
            last = self._last_item()
            if last is not None:
                self._queue.put(last)
            self._queue.put(None)
            self._thread.join()
        self._shutdown(joined)
        self._check()

    def _last_item(self):
        return None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
