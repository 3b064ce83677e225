"""The output side of the drivers that write pictures (predict_files.predict_from_files, annotation_labels.write_semantic_masks), for both
PNG encoders: Layout, the ONE place that knows where a batch's pictures, their streams and the streams' lengths lie; write_png, the host
encoder's writer task (png_device.write_stream is the device encoder's); PictureStage, the ONE hand-over of batches to the writer threads
of a preprocess.WriterRing.  No torch at import: the stage imports it when it is made."""
from __future__ import annotations

import contextlib
from typing import Optional, Sequence

import numpy as np

from . import png_device


class Layout:
    """The output buffers of a batch of sizes [(h, w)] * B and kinds [(c, mode, palette_bytes)]: pictures = [(h, w, c, mode, palette_bytes)]
    kind-major and image-minor, picture i = k * B + b being (kind k, image b).  Its u8 [h, w, c] bytes are raw_at[i] .. raw_at[i + 1] of the
    raw buffer (raw_bytes in all; a batch of one size has every kind as ONE [B, H, W(, c)] block: views(raw), of a tensor); with the device encoder its zlib
    stream has stream_at[i] .. stream_at[i + 1] of the stream buffer, png_device.stream_bound bytes, and its length is int32 word i of those
    at lengths_at, the streams' end rounded up to 4 bytes.  span(at, k): kind k's part of either buffer.  host_bytes[encoder] travel back:
    the raw buffer ("host"), or streams and lengths ("device").  max_segments[k]: kind k's largest png_device.segments."""

    def __init__(self, sizes: Sequence, kinds: Sequence):
        self.sizes, self.kinds = tuple((int(h), int(w)) for h, w in sizes), tuple(kinds)
        self.pictures = [(h, w, int(c), mode, palette_bytes) for c, mode, palette_bytes in self.kinds for h, w in self.sizes]
        self.key = tuple(p[:3] for p in self.pictures)                              # what the encoder's descriptor tables depend on
        self.raw_at = np.cumsum([0] + [h * w * c for h, w, c in self.key])
        self.stream_at = np.cumsum([0] + [png_device.stream_bound(*p) for p in self.key])
        self.raw_bytes, self.lengths_at = int(self.raw_at[-1]), (int(self.stream_at[-1]) + 3) // 4 * 4
        self.host_bytes = {"host": self.raw_bytes, "device": self.lengths_at + 4 * len(self.pictures)}
        self.max_segments = tuple(max(png_device.segments(h, w, c) for h, w in self.sizes) for c, _, _ in self.kinds)

    def span(self, at, k: int) -> slice:
        return slice(int(at[k * len(self.sizes)]), int(at[(k + 1) * len(self.sizes)]))

    def views(self, raw):
        (H, W), = set(self.sizes)                                                   # a batch of ONE size: ValueError otherwise
        return [raw[self.span(self.raw_at, k)].view((len(self.sizes), H, W) + ((c,) if c != 1 else ())) for k, (c, _, _) in enumerate(self.kinds)]


def write_png(path: str, a: np.ndarray, mode: str, palette_bytes: Optional[bytes], compress_level: int):
    """What a writer thread does with a raw picture: encode it with Pillow and write the file."""
    from PIL import Image
    im = Image.fromarray(a)                     # u8 [H, W] -> L, u8 [H, W, 3] -> RGB
    if palette_bytes is not None:
        im.putpalette(palette_bytes)            # L -> P: the bytes stay, the palette travels with them
    if im.mode != mode:
        raise ValueError(f"{path}: a mode {im.mode} image where {mode} was meant")
    im.save(path, format="PNG", compress_level=compress_level)


class PictureStage(contextlib.AbstractContextManager):
    """A preprocess.WriterRing of `n_writers` "zutis-write" threads and the hand-over of batches to it.  Per batch k: raw = take(k, layout,
    paths) — slot k % 2, once the writers of batch k - 2 are done; paths in the layout's picture order; raw: u8 [layout.raw_bytes] on the
    device —, the driver fills raw (or layout.views(raw)), commit().  commit(): with encoder "device" ONE ops.png_deflate per kind, raw ->
    stream buffer (each bracketed by a ("zh_png_deflate", e0, e1) entry of `events` when a list is given; its tables img_off, out_off int64
    [kinds, B], hw int32 [B, 2] go up in ONE copy per distinct layout and are kept for the last 64); the batch's ONE copy back into the
    slot's pinned buffer; the slot's event; then batch k - 1 goes to the writers, one task per picture, after THIS thread has waited for
    its event.  Leaving the `with` block hands the last batch over and waits for every writer (the first failure is raised) or, with an
    exception, cancels what has not started: no thread outlives it.  error: the RuntimeError's text for a length word outside 0 < n <=
    bound, formatted with path, h, w, c.  device None (encoder "host" only): CPU tensors stand for the device's."""

    def __init__(self, encoder: str, pin: bool, n_writers: int, device=None, *, compress_level: int = 1, events=None, error: str = "{path}"):
        import torch
        from . import _lib, preprocess
        if encoder == "device" and torch.device(device or "cpu").type != "cuda":
            raise _lib.ZutisHipError("PictureStage: png_encoder=\"device\" encodes on the GPU")
        self.encoder, self.device, self.compress_level, self.events, self.error = encoder, device, int(compress_level), events, error
        self.ring = preprocess.WriterRing(pin, n_writers, "zutis-write")
        self.raw, self.streams, self.tables = preprocess.DoubleBuffer(False, device), preprocess.DoubleBuffer(False, device), {}
        self.current = self.waiting = None      # (slot, host bytes, layout, paths, raw) of the batch being filled / whose copy back is in flight

    def __exit__(self, exc_type, *exc):
        with self.ring:                         # the pool is joined whatever happens
            if exc_type is None:
                self._hand_over()
                self.ring.drain()

    def take(self, k: int, layout: Layout, paths: Sequence[str]):
        host, _ = self.ring.take(k % 2, layout.host_bytes[self.encoder])           # waits for the writers of batch k - 2
        self.current = (k % 2, host, layout, paths, self.raw.take(k % 2, layout.raw_bytes))
        return self.current[4]

    def commit(self):
        import torch
        from . import ops
        slot, host, layout, _, out = self.current
        if self.encoder == "device":                                               # the pictures become their streams
            raw, out = out, self.streams.take(slot, layout.host_bytes["device"])
            K, B = len(layout.kinds), len(layout.sizes)
            if layout.key not in self.tables:                                      # the encoder's descriptors: ONE upload per distinct layout
                if len(self.tables) >= 64:
                    self.tables.clear()
                at = np.stack([layout.raw_at[:-1], layout.stream_at[:-1]]).astype(np.int64).reshape(2, K, B)
                up = torch.from_numpy(np.concatenate([(at - at[:, :, :1]).reshape(-1).view(np.uint8),       # offsets within the kind's span
                                                      np.asarray(layout.sizes, np.int32).reshape(-1).view(np.uint8)])).to(self.device)
                self.tables[layout.key] = (*up[:16 * K * B].view(torch.int64).view(2, K, B), up[16 * K * B:].view(torch.int32).view(B, 2))
            (img_off, out_off, hw), lengths = self.tables[layout.key], out[layout.lengths_at:].view(torch.int32).view(K, B)
            mark = lambda: None if self.events is None else torch.cuda.current_stream().record_event(torch.cuda.Event(enable_timing=True))  # noqa: E731
            for k, (c, _, _) in enumerate(layout.kinds):
                e0 = mark()
                ops.png_deflate(raw[layout.span(layout.raw_at, k)], img_off[k], hw, c, out[layout.span(layout.stream_at, k)], out_off[k], lengths[k],
                                layout.max_segments[k])
                if e0 is not None:
                    self.events.append(("zh_png_deflate", e0, mark()))
        host.copy_(out, non_blocking=True)                                         # every picture of the batch: ONE copy back
        if self.ring.events[slot] is not None:
            self.ring.events[slot].record()
        self._hand_over()                                                          # batch k - 1 is written while batch k is on the device
        self.waiting, self.current = self.current, None

    def _hand_over(self):
        if self.waiting is None:
            return
        (slot, host, layout, paths, _), self.waiting = self.waiting, None
        if self.ring.events[slot] is not None:
            self.ring.events[slot].synchronize()                                   # the bytes are in the pinned buffer
        a = host.numpy()
        lengths = a[layout.lengths_at:].view(np.int32) if self.encoder == "device" else None
        for i, (h, w, c, mode, palette_bytes) in enumerate(layout.pictures):
            if lengths is None:
                picture = a[layout.raw_at[i]:layout.raw_at[i + 1]].reshape((h, w) if c == 1 else (h, w, c))
                self.ring.submit(slot, write_png, paths[i], picture, mode, palette_bytes, self.compress_level)
                continue
            at, n = int(layout.stream_at[i]), int(lengths[i])
            if not 0 < n <= layout.stream_at[i + 1] - at:
                raise RuntimeError(self.error.format(path=paths[i], h=h, w=w, c=c))
            self.ring.submit(slot, png_device.write_stream, paths[i], a[at:at + n], h, w, mode, palette_bytes)
