"""``HipSuperResWorker`` -- the MI355X drop-in for the reference's RKNNLite ``SuperResWorker``
(server/lcm_sr_server.py:312-405): same constructor and ``upscale_once`` / ``upscale_bytes`` / ``close`` methods, with the tiled
numpy + NPU loop replaced by the HIP passes of ``superres.SuperResNet`` (csrc/sr.hip).  ``png`` output is written by
csrc/png.cpp; ``jpeg`` output by csrc/jpeg.hip + csrc/jpeg.cpp from the image on the device (LCM_JPEG_ENCODER=pil: by PIL).  A JPEG
*input* is decoded by csrc/jpeg_dec.cpp + csrc/jpeg_dec.hip straight into the device tensor the first pass reads
(LCM_JPEG_DECODER=pil, and every file the library does not support: by PIL, as every other format).  ``SuperResService`` builds
SR_NUM_WORKERS of these, each driven from its own thread: every worker has its own stream and workspace.  Install with
``server.lcm_sr_server.SuperResWorker = HipSuperResWorker``.  No CPU fallback: without a GPU the constructor
raises."""
from __future__ import annotations

import io
import os

import numpy as np
import torch

from ..lib import LcmHipError
from .. import superres as _sr
from .hip_worker import encode_png

FORMATS = ("png", "jpeg")


def _decode(image_bytes: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(image_bytes)).convert("RGB"))


def _pil_jpeg() -> bool:
    """LCM_JPEG_ENCODER=pil: the JPEG file comes from PIL on the host pixels, as before the library wrote it."""
    return os.environ.get("LCM_JPEG_ENCODER", "").lower() == "pil"


def _encode(rgb: np.ndarray, out_format: str, quality: int) -> bytes:
    if out_format == "jpeg":
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="JPEG", quality=int(quality))
        return buf.getvalue()
    return encode_png(rgb)


def _check_format(out_format: str) -> str:
    f = str(out_format).lower()
    if f not in FORMATS:
        raise RuntimeError(f"out_format must be 'png' or 'jpeg', got {out_format!r}")
    return f


class HipSuperResWorker:
    def __init__(self, worker_id: int, model_path: str, input_size: int, output_size: int):
        if not torch.cuda.is_available():
            raise LcmHipError("HipSuperResWorker needs an MI355X; no CPU fallback exists on this path")
        from .worker_factory import pick_device
        self.worker_id = worker_id
        self.model_path = model_path
        self.input_size = int(input_size)
        self.output_size = int(output_size)
        self.device = pick_device(worker_id, torch.cuda.device_count())      # LCM_DEVICES=all: worker i -> GPU i mod N
        self.net = _sr.SuperResNet(model_path, self.device, self.input_size, self.output_size)
        print(f"[SR] worker {self.worker_id} loaded {self.model_path} on {self.device}")

    def close(self):
        net, self.net = getattr(self, "net", None), None
        if net is not None:
            net.close()
            with torch.cuda.device(net.device):
                torch.cuda.empty_cache()

    def upscale_rgb(self, rgb: np.ndarray, magnitude: int = 1) -> np.ndarray:
        if self.net is None:
            raise RuntimeError("HipSuperResWorker is closed")
        return self.net.upscale_rgb(rgb, magnitude)

    def upscale_jpeg(self, rgb: np.ndarray, magnitude: int = 1, quality: int = 92) -> bytes:
        if self.net is None:
            raise RuntimeError("HipSuperResWorker is closed")
        return self.net.upscale_jpeg(rgb, magnitude, quality)

    def upscale_once(self, image_bytes: bytes, out_format: str = "png", quality: int = 92) -> bytes:
        return self._upscale(image_bytes, 1, _check_format(out_format), quality)

    def upscale_bytes(self, image_bytes: bytes, *, magnitude: int, out_format: str, quality: int) -> bytes:
        mag = _sr.check_magnitude(magnitude)
        return self._upscale(image_bytes, mag, _check_format(out_format), quality)

    def _upscale(self, image_bytes: bytes, mag: int, fmt: str, quality: int) -> bytes:
        lib_jpeg = fmt == "jpeg" and not _pil_jpeg()
        dev = None
        if self.net is not None:
            try:
                dev = self.net.decode_jpeg(image_bytes, mag)     # None: not a JPEG the library decodes -> PIL
            except RuntimeError:
                if lib_jpeg:
                    _sr.check_quality(quality)                   # a bad quality is reported before a size that is too large
                raise
        if dev is None:                                          # the path every input took before, in its order of checks
            if lib_jpeg:
                return self.upscale_jpeg(_decode(image_bytes), mag, quality)
            return _encode(self.upscale_rgb(_decode(image_bytes), mag), fmt, quality)
        if lib_jpeg:
            return self.net.upscale_device_jpeg(dev, mag, quality)
        return _encode(self.net.upscale_device_rgb(dev, mag), fmt, quality)
