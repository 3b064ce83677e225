"""The output side of the drivers that write pictures (predict_files.predict_from_files, annotation_labels.write_semantic_masks), for both
PNG encoders and both JPEG encoders: Layout, the ONE place that knows where a batch's pictures, their streams and the streams' lengths
lie; write_png / write_jpeg, the host encoders' writer tasks (png_device.write_stream / jpeg_device.write_scan are the device encoders');
PictureStage, the ONE hand-over of batches to the writer threads of a preprocess.WriterRing.  No torch at import: the stage imports it
when it is made."""
from __future__ import annotations

import contextlib
from typing import Optional, Sequence

import numpy as np

from . import jpeg_device, png_device


class Layout:
    """The output buffers of a batch of sizes [(h, w)] * B and kinds [(c, mode, palette_bytes)]: pictures = [(h, w, c, mode, palette_bytes)]
    kind-major and image-minor, picture i = k * B + b being (kind k, image b).  Its u8 [h, w, c] bytes are raw_at[i] .. raw_at[i + 1] of the
    raw buffer (raw_bytes in all; a batch of one size has every kind as ONE [B, H, W(, c)] block: views(raw), of a tensor); with the device encoder its zlib
    stream has stream_at[i] .. stream_at[i + 1] of the stream buffer, png_device.stream_bound bytes, and its length is int32 word i of those
    at lengths_at, the streams' end rounded up to 4 bytes.  span(at, k): kind k's part of either buffer.  host_bytes[encoder] travel back:
    the raw buffer ("host"), or streams and lengths ("device").  max_segments[k]: kind k's largest png_device.segments.
    A kind of mode "JPEG" (c = 3) is written as a baseline JPEG by `jpeg_encoder`, whatever the PNG encoder: "host" — its raw bytes travel
    (in the stream buffer too, at their own size), "device" — its scan travels at jpeg_device.scan_slot stride with its length word.
    forms[encoder][i]: what travels for picture i under PNG encoder `encoder` — "raw", "png" or "jpeg" —, at[encoder]: where (at["device"]
    is stream_at; at["host"] is raw_at unless a JPEG kind is encoded on the device), lengths[encoder]: the offset of the length words or
    None when nothing is encoded on the device."""

    def __init__(self, sizes: Sequence, kinds: Sequence, jpeg_encoder: str = "host"):
        self.sizes, self.kinds, self.jpeg_encoder = tuple((int(h), int(w)) for h, w in sizes), tuple(kinds), jpeg_encoder
        self.pictures = [(h, w, int(c), mode, palette_bytes) for c, mode, palette_bytes in self.kinds for h, w in self.sizes]
        if any(mode == "JPEG" and c != 3 for _, _, c, mode, _ in self.pictures):
            raise ValueError("picture_out.Layout: a JPEG kind has three channels")
        # what the encoders' descriptor tables depend on
        self.key = tuple(p[:3] + ((f"jpeg-{jpeg_encoder}",) if p[3] == "JPEG" else ()) for p in self.pictures)
        self.raw_at = np.cumsum([0] + [h * w * c for h, w, c, _, _ in self.pictures])
        self.raw_bytes = int(self.raw_at[-1])
        self.forms, self.at, self.lengths, self.host_bytes = {}, {}, {}, {}
        width = {"raw": lambda h, w, c: h * w * c, "png": png_device.stream_bound, "jpeg": lambda h, w, c: jpeg_device.scan_slot(h, w)}
        for encoder in png_device.ENCODERS:
            forms = [("jpeg" if jpeg_encoder == "device" else "raw") if mode == "JPEG" else ("png" if encoder == "device" else "raw")
                     for _, _, _, mode, _ in self.pictures]
            at = np.cumsum([0] + [width[f](h, w, c) for f, (h, w, c, _, _) in zip(forms, self.pictures)])
            encoded = any(f != "raw" for f in forms)
            self.forms[encoder], self.at[encoder] = forms, at
            self.lengths[encoder] = (int(at[-1]) + 3) // 4 * 4 if encoded or encoder == "device" else None
            self.host_bytes[encoder] = self.lengths[encoder] + 4 * len(self.pictures) if self.lengths[encoder] is not None else self.raw_bytes
        self.stream_at, self.lengths_at = self.at["device"], self.lengths["device"]
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


def write_jpeg(path: str, a: np.ndarray, quality: int, subsampling: str, pillow: bool = True):
    """What a writer thread does with a raw picture that becomes a JPEG: Pillow's encoder at the settings jpeg_device.encode_np defines
    (the same bytes), or, pillow=False (a Pillow without restart_marker_blocks), encode_np itself."""
    if not pillow:
        data = jpeg_device.encode_np(a, quality, subsampling)
        with open(path, "wb") as f:
            f.write(data)
        return
    from PIL import Image
    Image.fromarray(a).save(path, format="JPEG", quality=int(quality), subsampling=jpeg_device.SUBSAMPLINGS[subsampling],
                            restart_marker_blocks=jpeg_device.ENC_INTERVAL_MCUS)


class PictureStage(contextlib.AbstractContextManager):
    """A preprocess.WriterRing of `n_writers` "zutis-write" threads and the hand-over of batches to it.  Per batch k: raw = take(k, layout,
    paths) — slot k % 2, once the writers of batch k - 2 are done; paths in the layout's picture order; raw: u8 [layout.raw_bytes] on the
    device —, the driver fills raw (or layout.views(raw)), commit().  commit(): with encoder "device" ONE ops.png_deflate per kind, raw ->
    stream buffer (each bracketed by a ("zh_png_deflate", e0, e1) entry of `events` when a list is given; its tables img_off, out_off int64
    [kinds, B], hw int32 [B, 2] go up in ONE copy per distinct layout and are kept for the last 64); the batch's ONE copy back into the
    slot's pinned buffer; the slot's event; then batch k - 1 goes to the writers, one task per picture, after THIS thread has waited for
    its event.  Leaving the `with` block hands the last batch over and waits for every writer (the first failure is raised) or, with an
    exception, cancels what has not started: no thread outlives it.  error: the RuntimeError's text for a length word outside 0 < n <=
    bound, formatted with path, h, w, c.  device None (encoder "host" only): CPU tensors stand for the device's.
    Kinds of mode "JPEG" (the layouts are made with the stage's jpeg_encoder): "host" — a writer encodes the raw picture with Pillow
    (write_jpeg); "device" — ONE ops.jpeg_encode per such kind behind the zh_png_deflate calls (a ("zh_jpeg_encode", e0, e1) entry of
    `events` each), the scans travel in the batch's one copy back and a writer puts header and FF D9 around them (jpeg_device.write_scan).
    A scan whose length word exceeds its slot (the JPEG is larger than the pixels) did not fit: the handing-over thread copies that
    picture back from the raw slot — intact until batch k + 2 takes it — and gives it to the host arm: the same bytes; such pictures are
    counted in jpeg_host_fallbacks.  A length word <= 0 is the RuntimeError above.  zh_jpeg_encode takes ONE slot size a call: in a batch
    of several sizes every scan is held to the smallest picture's slot (the drivers that write JPEG kinds batch one size)."""

    def __init__(self, encoder: str, pin: bool, n_writers: int, device=None, *, compress_level: int = 1, events=None, error: str = "{path}",
                 jpeg_encoder: str = "host", jpeg_quality: int = 90, jpeg_subsampling: str = "4:2:0"):
        import torch
        from . import _lib, preprocess
        if encoder == "device" and torch.device(device or "cpu").type != "cuda":
            raise _lib.ZutisHipError("PictureStage: png_encoder=\"device\" encodes on the GPU")
        if jpeg_device.check_encoder("PictureStage", jpeg_encoder) == "device" and torch.device(device or "cpu").type != "cuda":
            raise _lib.ZutisHipError("PictureStage: jpeg_encoder=\"device\" encodes on the GPU")
        self.jpeg_sub = jpeg_device.check_encode_args("PictureStage", jpeg_quality, jpeg_subsampling)
        self.jpeg_encoder, self.jpeg_quality, self.jpeg_subsampling = jpeg_encoder, int(jpeg_quality), jpeg_subsampling
        self.jpeg_pillow, self.jpeg_host_fallbacks, self.jpeg_quant = None, 0, None
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
        if layout.jpeg_encoder != self.jpeg_encoder:
            raise ValueError(f"PictureStage: a layout made for jpeg_encoder {layout.jpeg_encoder!r} in a stage of {self.jpeg_encoder!r}")
        host, _ = self.ring.take(k % 2, layout.host_bytes[self.encoder])           # waits for the writers of batch k - 2
        self.current = (k % 2, host, layout, paths, self.raw.take(k % 2, layout.raw_bytes))
        return self.current[4]

    def commit(self):
        import torch
        from . import ops
        slot, host, layout, _, out = self.current
        forms, at = layout.forms[self.encoder], layout.at[self.encoder]
        if layout.lengths[self.encoder] is not None:                               # some pictures become their streams / scans
            raw, out = out, self.streams.take(slot, layout.host_bytes[self.encoder])
            K, B = len(layout.kinds), len(layout.sizes)
            tkey = (self.encoder, layout.key)
            if tkey not in self.tables:                                            # the encoders' descriptors: ONE upload per distinct layout
                if len(self.tables) >= 64:
                    self.tables.clear()
                offs = np.stack([layout.raw_at[:-1], at[:-1]]).astype(np.int64).reshape(2, K, B)
                up = torch.from_numpy(np.concatenate([(offs - offs[:, :, :1]).reshape(-1).view(np.uint8),   # offsets within the kind's span
                                                      np.asarray(layout.sizes, np.int32).reshape(-1).view(np.uint8)])).to(self.device)
                self.tables[tkey] = (*up[:16 * K * B].view(torch.int64).view(2, K, B), up[16 * K * B:].view(torch.int32).view(B, 2))
            (img_off, out_off, hw), lengths = self.tables[tkey], out[layout.lengths[self.encoder]:].view(torch.int32).view(K, B)
            mark = lambda: None if self.events is None else torch.cuda.current_stream().record_event(torch.cuda.Event(enable_timing=True))  # noqa: E731
            for k, (c, _, _) in enumerate(layout.kinds):
                if forms[k * B] != "png":
                    continue
                e0 = mark()
                ops.png_deflate(raw[layout.span(layout.raw_at, k)], img_off[k], hw, c, out[layout.span(at, k)], out_off[k], lengths[k],
                                layout.max_segments[k])
                if e0 is not None:
                    self.events.append(("zh_png_deflate", e0, mark()))
            for k in range(K):
                if forms[k * B] == "raw":                                          # a picture the host encodes travels as it is
                    out[layout.span(at, k)].copy_(raw[layout.span(layout.raw_at, k)])
                elif forms[k * B] == "jpeg":
                    if self.jpeg_quant is None:
                        self.jpeg_quant = jpeg_device.quant_tensor(self.jpeg_quality, self.device)
                    hs = 16 if self.jpeg_sub == 2 else 8
                    e0 = mark()
                    ops.jpeg_encode(raw[layout.span(layout.raw_at, k)], img_off[k], hw, self.jpeg_sub, self.jpeg_quant, out[layout.span(at, k)], out_off[k],
                                    min(jpeg_device.scan_slot(h, w) for h, w in layout.sizes), lengths[k], max(-(-h // hs) * -(-w // hs) for h, w in layout.sizes))
                    if e0 is not None:
                        self.events.append(("zh_jpeg_encode", e0, mark()))
        host.copy_(out, non_blocking=True)                                         # every picture of the batch: ONE copy back
        if self.ring.events[slot] is not None:
            self.ring.events[slot].record()
        self._hand_over()                                                          # batch k - 1 is written while batch k is on the device
        self.waiting, self.current = self.current, None

    def _hand_over(self):
        if self.waiting is None:
            return
        (slot, host, layout, paths, raw), self.waiting = self.waiting, None
        if self.ring.events[slot] is not None:
            self.ring.events[slot].synchronize()                                   # the bytes are in the pinned buffer
        a = host.numpy()
        forms, at = layout.forms[self.encoder], layout.at[self.encoder]
        lengths = a[layout.lengths[self.encoder]:].view(np.int32) if layout.lengths[self.encoder] is not None else None
        for i, (h, w, c, mode, palette_bytes) in enumerate(layout.pictures):
            lo, n = int(at[i]), int(lengths[i]) if forms[i] != "raw" else 0
            if forms[i] == "raw":
                picture = a[lo:lo + h * w * c].reshape((h, w) if c == 1 else (h, w, c))
                if mode == "JPEG":
                    self._write_jpeg(slot, paths[i], picture)
                else:
                    self.ring.submit(slot, write_png, paths[i], picture, mode, palette_bytes, self.compress_level)
            elif n <= 0 or (forms[i] == "png" and n > at[i + 1] - lo):
                raise RuntimeError(self.error.format(path=paths[i], h=h, w=w, c=c))
            elif forms[i] == "png":
                self.ring.submit(slot, png_device.write_stream, paths[i], a[lo:lo + n], h, w, mode, palette_bytes)
            elif n > min(jpeg_device.scan_slot(*size) for size in layout.sizes):   # the scan did not fit: the raw picture, synchronously, to the host arm
                self.jpeg_host_fallbacks += 1
                self._write_jpeg(slot, paths[i], raw[int(layout.raw_at[i]):int(layout.raw_at[i + 1])].cpu().numpy().reshape(h, w, 3))
            else:
                self.ring.submit(slot, jpeg_device.write_scan, paths[i], a[lo:lo + n], h, w, self.jpeg_quality, self.jpeg_subsampling)

    def _write_jpeg(self, slot, path, picture):
        if self.jpeg_pillow is None:
            self.jpeg_pillow = jpeg_device.pillow_writes_restart_blocks()
        self.ring.submit(slot, write_jpeg, path, picture, self.jpeg_quality, self.jpeg_subsampling, self.jpeg_pillow)
