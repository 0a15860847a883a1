"""``HipLcmWorker`` -- the MI355X drop-in for the reference's ``DiffusersCudaWorker``
(backends/cuda_worker.py:20-304): same constructor, attributes, ``run_job`` /
``run_job_with_latents`` contract and error behaviour, with the arithmetic of
``self.pipe(...)`` (cuda_worker.py:221-229) replaced by the hipGraph of HIP kernels in
``pipeline.LcmHipPipeline``.

Env (as the reference, backends/cuda_worker.py:43-61):
  MODEL_ROOT, MODEL   checkpoint location (diffusers directory or single .safetensors file).  MODEL=synthetic (or
                      LCM_HIP_SYNTHETIC=1) selects seeded synthetic weights of the SD1.5 architecture, MODEL=synthetic-sd2
                      those of SD 2.1-768 (865 M UNet, OpenCLIP-H text tower, v-prediction schedule) --
                      no checkpoint ships with the reference.
  LCM_PREDICTION_TYPE        epsilon | v_prediction | sample: overrides the prediction type guessed for a single-file
                             checkpoint (weights.single_file_prediction_type; e.g. epsilon for SD 2.x-base)
  CUDA_DEVICE / HIP_DEVICE   default cuda:0 (torch's name for the HIP device)
  LCM_REFINE_CACHE_MB        device-resident cache of refinement latents (denoise_strength / pass_number requests), MB per
                             engine; default 64, 0 turns it off
  LCM_RESIZE                 hip (default) | pil: where an upload of another size than the request's is fitted -- the HIP Lanczos
                             resampler on the lane's stream, or PIL on the caller's thread; the bytes are the same (backends/fit.py)
  LCM_SAMPLERS               request (default) | lcm: whether ``sampler_name`` / ``scheduler`` are read (backends/sampler.py); with lcm
                             every request is stepped by the LCM sampler, as before the fields were known
  LCM_SDUPSCALE_MAX_TILES    the most tiles an SD-upscale request (``script_name``, backends/sdupscale.py) may have; default 64
  CUDA_DTYPE                 fp16 (default).  bf16 / fp32 -- which the reference honours -- are REFUSED unless LCM_HIP_DTYPE=fp16
                             says to run them in this backend's one arithmetic (fp16 operands, fp32 accumulation)
"""
from __future__ import annotations

import io
import os
import struct
import threading
import weakref
import zlib
from typing import Tuple

import numpy as np
import torch

from ..lib import LcmHipError
from ..pipeline import LcmHipPipeline, draw_noise, draw_noise_hires, draw_noise_img2img, draw_variation_sources
from ..prompt import HipPromptEncoder
from ..scheduler import LCMSchedule
from .. import weights as _weights
from . import controlnet as _controlnet
from . import fit as _fit
from . import hires as _hires
from . import img2img as _img2img
from . import inpaint as _inpaint
from . import prompt_syntax as _prompt
from . import refine as _refine
from . import sampler as _sampler
from . import sdupscale as _sdupscale
from . import variation as _variation


def parse_size(size) -> Tuple[int, int]:
    try:
        w_str, h_str = str(size).lower().split("x")
        return int(w_str), int(h_str)
    except Exception:
        raise RuntimeError(f"Invalid size '{size}', expected 'WIDTHxHEIGHT'")     # cuda_worker.py:204-208


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


_PNG_POOL = None
_PNG_POOL_LOCK = threading.Lock()


def _png_pool(n):
    """Stripe-deflate threads.  The stripe COUNT of an image (and so its bytes) follows LCM_PNG_THREADS alone; the pool is
    wider (up to the host's cores, at most 16) so that the images of a drained batch deflate side by side."""
    global _PNG_POOL
    n = max(n, min(16, os.cpu_count() or 1))
    with _PNG_POOL_LOCK:
        if _PNG_POOL is None or _PNG_POOL._max_workers < n:
            from concurrent.futures import ThreadPoolExecutor
            _PNG_POOL = ThreadPoolExecutor(max_workers=n, thread_name_prefix="lcm-png")
        return _PNG_POOL


_FINISH_POOL = None


def _finish_pool():
    """Threads that finish the jobs a ``run_job`` call drained from the pool's queue (PNG encode, set the job's future,
    ``task_done``).  Separate from the stripe pool: a finisher blocks on its image's stripes."""
    global _FINISH_POOL
    with _PNG_POOL_LOCK:
        if _FINISH_POOL is None:
            from concurrent.futures import ThreadPoolExecutor
            _FINISH_POOL = ThreadPoolExecutor(max_workers=min(16, max(4, os.cpu_count() or 4)), thread_name_prefix="lcm-finish")
        return _FINISH_POOL


def _deflate_stripe(args):
    buf, level, last = args
    co = zlib.compressobj(level, zlib.DEFLATED, -15)          # raw deflate: the stripes share one zlib wrapper
    return co.compress(buf) + co.flush(zlib.Z_FINISH if last else zlib.Z_FULL_FLUSH)


def encode_png(rgb) -> bytes:
    """uint8 [H,W,3] -> PNG file bytes (the reference's ``img.save(buf, format="PNG")``, cuda_worker.py:234-239).

    With the sampler at ~20 ms the PIL encoder (40-70 ms for 512x512) would dominate run_job, so the file is written by the
    library's own writer (csrc/png.cpp, ``lcm_png_encode_rgb8``): scanline filter "Up", one dynamic-Huffman deflate block per
    stripe over literals and distance-1 runs, LCM_PNG_THREADS stripes (default 8) compressed in parallel, Adler-32 / CRC-32
    combined from the stripes -- lossless, deterministic (the bytes depend on the image and the stripe count, not on timing),
    0.4 ms for 512x512 where zlib level 1 on 8 threads took 3 ms and PIL 40-70.
    LCM_PNG_ENCODER=zlib: the round-3 writer (numpy filter + zlib level LCM_PNG_COMPRESS on a Python thread pool, pigz-style
    stripes); =pil: PIL."""
    enc = os.environ.get("LCM_PNG_ENCODER", "").lower()
    if enc == "pil":
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="PNG", compress_level=int(os.environ.get("LCM_PNG_COMPRESS", "6")))
        return buf.getvalue()
    if enc != "zlib":
        import ctypes
        from .. import lib as _lib
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w, c = rgb.shape
        if c != 3:
            raise ValueError(f"encode_png expects RGB, got {c} channels")
        L = _lib.load()
        nthr = max(1, int(os.environ.get("LCM_PNG_THREADS", "8")))
        stripes = min(nthr, max(1, h // 64))                   # stripes of at least 64 scanlines
        cap = int(L.lcm_png_bound(w, h, stripes))
        out = np.empty(cap, np.uint8)
        n = ctypes.c_longlong(0)
        _lib.check(L.lcm_png_encode_rgb8(rgb.ctypes.data, w, h, w * 3, stripes, out.ctypes.data, cap, ctypes.byref(n)),
                   "lcm_png_encode_rgb8")
        return out[:n.value].tobytes()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, c = rgb.shape
    if c != 3:
        raise ValueError(f"encode_png expects RGB, got {c} channels")
    flat = rgb.reshape(h, w * 3)
    raw = np.empty((h, 1 + w * 3), np.uint8)
    raw[:, 0] = 2                      # filter type Up
    raw[0, 1:] = flat[0]
    np.subtract(flat[1:], flat[:-1], out=raw[1:, 1:])      # uint8 wrap-around == mod 256
    level = int(os.environ.get("LCM_PNG_COMPRESS", "1"))
    nthr = max(1, int(os.environ.get("LCM_PNG_THREADS", "8")))
    nstripes = min(nthr, max(1, h // 64))                  # stripes of at least 64 scanlines
    if nstripes == 1:
        comp = zlib.compress(raw.tobytes(), level)
    else:
        mv = memoryview(raw).cast("B")
        row = 1 + w * 3
        cuts = [(h * i // nstripes) * row for i in range(nstripes + 1)]
        parts = list(_png_pool(nthr).map(_deflate_stripe, [(mv[cuts[i]:cuts[i + 1]], level, i == nstripes - 1) for i in range(nstripes)]))
        comp = b"\x78\x01" + b"".join(parts) + struct.pack(">I", zlib.adler32(mv) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + _png_chunk(b"IDAT", comp) + _png_chunk(b"IEND", b""))


_JPEG_ENCODERS = {}
_JPEG_LOCK = threading.Lock()


def encode_jpeg(rgb, quality: int = 92) -> bytes:
    """uint8 [H,W,3] host pixels -> baseline 4:2:0 JPEG file bytes (the reference's ``img.save(buf, format="JPEG",
    quality=q)``, server/lcm_sr_server.py): the pixels are uploaded to the current device, ``lcm_jpeg_dct_rgb8``
    (csrc/jpeg.hip) turns them into quantised coefficients there and ``lcm_jpeg_encode_coefs`` (csrc/jpeg.cpp) writes the file
    on LCM_JPEG_THREADS host threads (default 8; the bytes do not depend on it).  Callers whose image is already on the device
    use ``superres.JpegEncoder`` directly.  One encoder per device, one call at a time.  LCM_JPEG_ENCODER=pil: PIL."""
    if os.environ.get("LCM_JPEG_ENCODER", "").lower() == "pil":
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="JPEG", quality=int(quality))
        return buf.getvalue()
    from .. import superres as _sr
    q = _sr.check_quality(quality)
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"encode_jpeg expects uint8 [H][W][3], got shape {rgb.shape}")
    if not torch.cuda.is_available():
        raise LcmHipError("encode_jpeg needs an MI355X; no CPU fallback exists on this path (LCM_JPEG_ENCODER=pil uses PIL)")
    dev = torch.device("cuda", torch.cuda.current_device())
    with _JPEG_LOCK:
        enc = _JPEG_ENCODERS.get(dev)
        if enc is None:
            enc = _JPEG_ENCODERS[dev] = _sr.JpegEncoder(dev)
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            src = torch.from_numpy(rgb).to(dev)
        return enc.encode_device(src, q, stream)


_JPEG_DECODERS = {}


def decode_jpeg(data) -> np.ndarray:
    """JPEG file bytes -> uint8 [H,W,3] host pixels, equal to ``np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))``: the
    markers and the entropy decoding on LCM_JPEG_THREADS host threads (csrc/jpeg_dec.cpp), the inverse DCT, chroma upsampling
    and colour conversion on the current device (csrc/jpeg_dec.hip).  Files the library does not decode (progressive, CMYK,
    ... -- include/lcm_hip.h), corrupt ones, and everything under LCM_JPEG_DECODER=pil go to PIL.  Callers that want the pixels
    on the device use ``superres.JpegDecoder`` directly.  One decoder per device, one call at a time."""
    from .. import superres as _sr

    def pil():
        from PIL import Image
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    mode = _sr.jpeg_decoder_mode()
    if mode == "pil" or bytes(data[:2]) != b"\xff\xd8":
        return pil()
    if not torch.cuda.is_available():
        raise LcmHipError("decode_jpeg needs an MI355X; no CPU fallback exists on this path (LCM_JPEG_DECODER=pil uses PIL)")
    dev = torch.device("cuda", torch.cuda.current_device())
    with _JPEG_LOCK:
        dec = _JPEG_DECODERS.get(dev)
        if dec is None:
            dec = _JPEG_DECODERS[dev] = _sr.JpegDecoder(dev)
        stream = torch.cuda.current_stream(dev)
        out = dec.decode_device(data, stream, 0, mode)
        if out is not None:
            with torch.cuda.device(dev), torch.cuda.stream(stream):
                host = out.cpu()
            stream.synchronize()
            return host.numpy()
    return pil()


def canny(rgb, low=100, high=200) -> np.ndarray:
    """uint8 [H,W,3] (or [B,H,W,3]) host pixels -> the Canny edge picture of the same shape, every pixel 0,0,0 or 255,255,255,
    as include/lcm_hip.h defines it (written after ``cv2.Canny(rgb, low, high)``; equality with OpenCV is unverified): the
    pixels are uploaded to the current device, ``lcm_canny_rgb8`` (csrc/canny.hip) runs there and the map is read back.  A
    request that wants the map as its ControlNet hint sends the photo with ``controlnet_module="canny"`` instead and nothing
    comes back to the host.  No CPU fallback."""
    from .. import ops as _ops
    a = np.ascontiguousarray(rgb)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3 or min(a.shape) < 1:
        raise ValueError(f"canny expects uint8 [H][W][3] or [B][H][W][3], got {a.dtype} {tuple(a.shape)}")
    low, high = float(low), float(high)
    if not (abs(low) < 1e9 and abs(high) < 1e9):
        raise ValueError(f"canny thresholds must be finite numbers, got {low!r}, {high!r}")
    if not torch.cuda.is_available():
        raise LcmHipError("canny needs an MI355X; no CPU fallback exists on this path")
    B, H, W = (1,) + a.shape[:2] if a.ndim == 3 else a.shape[:3]
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        src = torch.from_numpy(a.reshape(B, H, W, 3)).to(dev)
        ws = torch.empty(_ops.canny_ws_bytes(B, H, W), dtype=torch.uint8, device=dev)
        _ops.canny_rgb8(src, src, ws, B, H, W, low, high)
        host = src.cpu()
    return host.numpy().reshape(a.shape)


def resize(img, width, height, mode=0) -> np.ndarray:
    """uint8 [H,W] or [H,W,3] host pixels -> the picture fitted to width x height under ``resize_mode`` ``mode`` (0 just resize,
    1 crop and resize, 2 resize and fill; backends/fit.py), with the bytes of PIL's ``Image.resize(..., Image.LANCZOS)``: the
    pixels are uploaded to the current device, ``lcm_resize_lanczos_u8`` (csrc/resize.hip) computes the request's window there
    and it is read back.  A picture that already has the size comes back as it is.  Pictures outside the device path's domain
    (``fit.in_domain``: sides above 8192 / 4096, taller than 100 x their width) and everything under LCM_RESIZE=pil go to PIL.
    A request that carries its upload at another size needs no call: the worker fits it on its lane's stream."""
    from .. import ops as _ops
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or min(a.shape) < 1:
        raise ValueError(f"resize expects uint8 [H][W] or [H][W][3], got {a.dtype} {tuple(a.shape)}")
    width, height, mode = int(width), int(height), int(mode)
    if mode not in _fit.MODES:
        raise ValueError(f"resize mode {mode!r}: expected one of {sorted(_fit.MODES)}")
    if width < 1 or height < 1:
        raise ValueError(f"resize to {width}x{height}")
    f = _fit.prepare(a, width, height, mode)
    if not _fit.is_pending(f):
        return f
    if not torch.cuda.is_available():
        raise LcmHipError("resize needs an MI355X on this path (LCM_RESIZE=pil uses PIL)")
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev)
    win = (f.x0, f.y0, width, height)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        src = torch.from_numpy(a).to(dev)
        dst = torch.empty(f.shape, dtype=torch.uint8, device=dev)
        ws = torch.empty(_ops.resize_ws_bytes(a.shape[1], a.shape[0], 1 if a.ndim == 2 else 3, f.fit_w, f.fit_h, win),
                         dtype=torch.uint8, device=dev)
        _ops.resize_lanczos_u8(src, dst, ws, f.fit_w, f.fit_h, win)
        host = dst.cpu()
    return host.numpy()


def samplers():
    """What ``/sdapi/v1/samplers`` answers: [{"name", "aliases", "options"}], LCM first (the reference answers LCM alone,
    server/compat_endpoints.py:132-135), then the names ``sampler_name`` serves.  With LCM_SAMPLERS=lcm: LCM alone."""
    from .. import samplers as _s
    full = _s.sampler_list()
    return full if _sampler.mode() == "request" else full[:1]


def _rows(x, idx, n):
    """The per-request conditioning rows ``idx`` of a batch of n: tensors with n leading rows are gathered, tuples (SDXL's
    ``added``) and dicts walked, anything else passed through; the whole batch in order is returned as it is."""
    if list(idx) == list(range(n)):
        return x
    if isinstance(x, torch.Tensor) and x.dim() > 0 and x.shape[0] == n:
        return x[idx]
    if isinstance(x, tuple):
        return tuple(_rows(y, idx, n) for y in x)
    if isinstance(x, dict):
        return {k: _rows(v, idx, n) for k, v in x.items()}
    return x


def _take(res, out, idx):
    """The pipeline's result dict of the items ``idx`` -> their (rgb, pool8 row) slots of ``res``."""
    for b, i in enumerate(idx):
        res[i] = (out["rgb"][b], out["pool8"][b:b + 1])
    return res


class _Engine:
    """Everything resident for one (family, device, checkpoint): the pipeline (weights, launch plans, captured graphs), the
    text encoders, the style adapters and the micro-batching dispatcher.  The reference builds one pipeline -- and one
    weight copy -- per worker object (``DiffusersCudaWorker.__init__``, backends/cuda_worker.py:41-121; its ``WorkerPool`` creates
    exactly one, ``worker_id=0``, backends/worker_pool.py:228; the legacy ``PipelineService`` one per ``NUM_WORKERS``,
    forced to 1 on CUDA, server/lcm_sr_server.py:190-193).  Here the workers a caller creates for one GPU share one engine,
    so N threads blocking in ``run_job`` become batched passes -- and behind the single-consumer ``WorkerPool`` the batch comes
    from draining the pool's queue (``HipLcmWorker._drain``).  LCM_SHARE_ENGINE=0: one engine per worker.

    Lifetime: workers hold the engine, the engine never holds a worker, the registry and the dispatcher thread hold it
    weakly.  The pool's teardown -- ``del worker; gc.collect(); torch.cuda.empty_cache()`` (backends/worker_pool.py:270-276),
    no ``close()`` -- therefore releases the weights, plans, graphs and pinned buffers of the mode being unloaded."""

    def __init__(self, family_cls):
        self.family_cls = family_cls
        self.refs = 0
        self.batcher = None
        self.batch_sizes = (1,)
        self.active_style = None
        self.pipe = None
        self.encode = None           # SD1.5: HipPromptEncoder
        self.enc, self.tok = [], []  # SDXL: two encoders / tokenizers
        self.styles = {}
        self.device = None
        self.dtype = torch.float16
        self.timing = [] if os.environ.get("LCM_WORKER_TIMING", "0") == "1" else None
        # Lanes: sampler instances of the pipeline that run concurrently (own stream, scratch, graphs, text-encoder
        # buffers; shared weights).  Two batch-1 passes in flight take ~1.4x the time of one, so at low load -- where
        # nothing queues up to be coalesced -- the second lane is worth ~45 % more images/s.  LCM_LANES=1: one at a time.
        self.n_lanes = max(1, int(os.environ.get("LCM_LANES", "2") or 1))
        self.lane_locks = [threading.Lock() for _ in range(self.n_lanes)]
        self.lane_encoders = {}      # lane -> per-lane views of the text encoders
        self._style_cv = threading.Condition()
        self._style_users = 0        # passes currently running with `active_style` merged into the shared weights
        # refinement requests (denoise_strength / pass_number): the denoised latents x^k of every pass they run stay on the
        # device so that pass p of a request starts from its pass p - 1.  Plain requests never touch it.
        self.refine_cache = _refine.RefineCache(_refine.cache_bytes_from_env())
        self._stats_lock = threading.Lock()
        self.stats = dict(unet_evals=0, refine_cache_hits=0, refine_cache_misses=0, refine_cache_puts=0, controlnet_evals=0,
                          hires_requests=0, img2img_requests=0, inpaint_requests=0, controlnet_preprocessed=0,
                          resized_on_device=0, prompt_chunks=0, weighted_prompts=0, variation_requests=0, sampler_requests=0,
                          sdupscale_requests=0, sdupscale_tiles=0)
        # ControlNet: where it comes from (CONTROLNET=<dir or file> | "synthetic" | None); loaded on the first request that
        # carries a hint, released with the pipeline
        self.controlnet_src = None
        self.synthetic_model = False
        self._controlnet_lock = threading.Lock()

    def ensure_controlnet(self):
        """Load the ControlNet on first use.  RuntimeError when none is configured, when this family has none (SDXL) or when it
        does not fit the UNet."""
        pipe = self.pipe
        if pipe is None:
            raise RuntimeError("worker engine is closed")
        if not self.family_cls.CONTROLNET_OK:
            raise RuntimeError("controlnet_image: SDXL ControlNets are not supported by this worker (SD1.5 and SD 2.x only)")
        if pipe.controlnet is not None:
            return
        if not self.controlnet_src:
            raise RuntimeError("controlnet_image was sent but no ControlNet is loaded (set CONTROLNET=<dir or .safetensors file>)")
        with self._controlnet_lock:
            if pipe.controlnet is None:
                sd, cfg = _controlnet.load_controlnet_source(self.controlnet_src, pipe.unet.cfg, self.synthetic_model)
                pipe.set_controlnet(sd, cfg)

    def ensure_vae_encoder(self):
        """Build the VAE encoder on first use (image-to-image).  RuntimeError for a family that has none (SDXL) or a checkpoint
        without encoder tensors."""
        pipe = self.pipe
        if pipe is None:
            raise RuntimeError("worker engine is closed")
        if not self.family_cls.IMG2IMG_OK:
            raise RuntimeError("init_image: image-to-image is not served by the SDXL worker (SD1.5 and SD 2.x only)")
        pipe.lane_vae_encoder(pipe.lanes[0])         # LcmHipError (a RuntimeError) when the checkpoint has no encoder

    # ---- style LoRAs (backends/cuda_worker.py:123-196) -----------------------------------------
    def _want_style(self, style_id, level):
        from .styles import STYLE_REGISTRY
        if style_id and int(level) > 0 and style_id in self.styles:
            return (style_id, STYLE_REGISTRY[style_id].weight_for(level))
        return None

    def apply_style(self, style_id, level, stream=None):
        """Exclusive style selection; level 0 / unknown style = off.  Re-merges only when the selection changes."""
        want = self._want_style(style_id, level)
        if want == self.active_style:
            return
        with torch.cuda.stream(stream or self.pipe.stream):
            if self.active_style is not None and (want is None or want[0] != self.active_style[0]):
                self.styles[self.active_style[0]].apply(0.0)
            if want is not None:
                self.styles[want[0]].apply(want[1])
            torch.cuda.current_stream().synchronize()     # the merge must have landed before any lane replays a graph
        self.active_style = want

    def _enter_style(self, style_id, level, stream):
        """The merged weights are shared by all lanes: a pass may start when the style it needs is the merged one, or
        when no other pass is running (then it re-merges)."""
        want = self._want_style(style_id, level)
        with self._style_cv:
            while True:
                if want == self.active_style:
                    break
                if self._style_users == 0:
                    self.apply_style(style_id, level, stream)
                    break
                self._style_cv.wait()
            self._style_users += 1

    def _leave_style(self):
        with self._style_cv:
            self._style_users -= 1
            self._style_cv.notify_all()

    def _lane_encoders(self, lane):
        """(encode callable | None, [encoder views]) of a lane: same weights, activation buffers of their own."""
        e = self.lane_encoders.get(lane)
        if e is None:
            if lane == 0:
                e = (self.encode, list(self.enc))
            else:
                enc = None
                if self.encode is not None:
                    import copy
                    enc = copy.copy(self.encode)
                    enc.enc = self.encode.enc.view()
                e = (enc, [x.view() for x in self.enc])
            self.lane_encoders[lane] = e
        return e

    def run_batch(self, key, items, lane=0):
        """One batched sampler pass for ``items`` = [(req, seed[, noise])], all of ``key``, on lane ``lane``;
        -> per-item (rgb, pool8 row)."""
        key, n_ctx = _prompt.split_ctx(key)          # a long-prompt pass: the kind's own key + ("ctx", n)
        key, sdu = _sdupscale.split_key(key)         # SD-upscale jobs: the image-to-image key + ("sdupscale", overlap, upscaler, W, H)
        key, smp = _sampler.split_key(key)           # a sampler pass: the kind's own key + ("sampler", name, sigmas); None: LCM
        smp_kw = dict(sampler=smp) if smp is not None else {}
        width, height, steps, g, style_id, level = key[:6]
        import time as _t
        t0 = _t.perf_counter()
        lane = lane % self.n_lanes
        with self.lane_locks[lane]:                  # a lane (stream, scratch, graphs) runs one pass at a time
            pipe = self.pipe
            if pipe is None:
                raise RuntimeError("worker engine is closed")
            stream = pipe.lane(lane).stream
            self._enter_style(style_id, level, stream)   # lazy: no re-merge while consecutive batches use the same style
            try:
                reqs = [it[0] for it in items]
                with torch.cuda.stream(stream):
                    pe, kw = self.family_cls._conditioning(self, reqs, width, height, g, lane, **({"n_ctx": n_ctx} if n_ctx > 1 else {}))
                t1 = _t.perf_counter()
                noises = [it[2] for it in items] if all(len(it) > 2 and it[2] is not None for it in items) else None
                seeds = [it[1] for it in items]
                # variation seeds / seed-resize are per image, like the prompt: items that carry one (VariedItem, _with_variation)
                # share the pass with plain ones, and a pass without any gets no variation= at all
                varied = [getattr(it, "variation", None) for it in items]
                var_kw = (lambda idx: dict(variation=[varied[i] for i in idx])) if any(v is not None for v in varied) else (lambda idx: {})
                if _hires.is_hires_key(key):         # key = plain key + (KEY_TAG, target width, target height, hr_steps, strength, mode)
                    tw, th, hr_steps, strength, mode = key[7:12]
                    cap = pipe.hires_batch_cap(tw, th, hr_steps, strength, g, lane=lane, sizes=self.batch_sizes, n_ctx=n_ctx)
                    res = self._run_capped(items, noises, pe, kw, cap, stream, "hires_requests", lambda idx, sub_pe, sub_noises, sub_kw:
                                           pipe.generate(sub_pe, [seeds[i] for i in idx], width, height, steps, g, noises=sub_noises,
                                                         lane=lane, hires=(tw, th, hr_steps, strength, mode), **var_kw(idx), **sub_kw))
                elif sdu is not None:                # SD upscale: the jobs one after the other, each its tiles' passes + the combine
                    cap = pipe.img2img_batch_cap(width, height, steps, key[7], g, lane=lane, sizes=self.batch_sizes, n_ctx=n_ctx, **smp_kw)
                    res, done = [None] * len(items), {}
                    for i, it in enumerate(items):
                        if id(it) not in done:       # (a repeated item filled the plan size: served once)
                            done[id(it)] = self._run_sdupscale(pipe, it, i, len(items), pe, kw, cap, lane, stream,
                                                               (width, height, steps, key[7], g), smp_kw)
                        res[i] = done[id(it)]
                elif _img2img.is_img2img_key(key):   # key = plain key + (KEY_TAG, strength); items carry the fitted picture
                    cap = pipe.img2img_batch_cap(width, height, steps, key[7], g, lane=lane, sizes=self.batch_sizes, n_ctx=n_ctx, **smp_kw)
                    res = self._run_capped(items, noises, pe, kw, cap, stream, "img2img_requests", lambda idx, sub_pe, sub_noises, sub_kw:
                                           pipe.generate_img2img(sub_pe, [seeds[i] for i in idx], _fit.stack([items[i][3] for i in idx]),
                                                                 width, height, steps, key[7], g, noises=sub_noises, lane=lane, **smp_kw,
                                                                 **sub_kw))
                elif _inpaint.is_inpaint_key(key):   # key = plain key + (KEY_TAG, strength, mask_blur); items carry picture and mask
                    cap = pipe.inpaint_batch_cap(width, height, steps, key[7], g, lane=lane, sizes=self.batch_sizes, n_ctx=n_ctx)
                    res = self._run_capped(items, noises, pe, kw, cap, stream, "inpaint_requests", lambda idx, sub_pe, sub_noises, sub_kw:
                                           pipe.generate_inpaint(sub_pe, [seeds[i] for i in idx], _fit.stack([items[i][3] for i in idx]),
                                                                 _fit.stack([items[i][4] for i in idx]), width, height, steps, key[7],
                                                                 key[8], g, noises=sub_noises, lane=lane, **sub_kw))
                elif len(key) > 6 and not _controlnet.is_control_key(key):
                    res = self._run_refine(pipe, key, items, noises, pe, kw, lane, stream, var_kw)
                else:                                # plain, or ControlNet: the hints ride along, the scale is key[7]
                    control = _controlnet.is_control_key(key)
                    pre = _controlnet.key_preprocessor(key) if control else ()
                    if control:
                        kw = dict(kw, control=(_fit.stack([it[3] for it in items]), key[7]))
                        if pre:                          # a photo: the edge map is made on the device, ahead of the hint stack
                            kw["preprocess"] = pre
                    out = pipe.generate(pe, seeds, width, height, steps, g, noises=noises, lane=lane, **var_kw(range(len(items))), **smp_kw,
                                        **kw)
                    res = _take([None] * len(items), out, range(len(items)))
                    with self._stats_lock:
                        self.stats["unet_evals"] += steps
                        self.stats["controlnet_evals"] += steps if control else 0
                        self.stats["controlnet_preprocessed"] += len(items) if pre else 0
                # requests of this batch with an upload that the device fitted (LCM_RESIZE=hip): the pipeline's upload() ran the
                # resampler into their slots
                fitted = len({id(it) for it in items if any(_fit.is_pending(x) for x in it[3:])})
                if fitted:
                    with self._stats_lock:
                        self.stats["resized_on_device"] += fitted
                if smp is not None:
                    with self._stats_lock:
                        self.stats["sampler_requests"] += len({id(it) for it in items})
                n_varied = len({id(it) for it, v in zip(items, varied) if v is not None})
                if n_varied:
                    with self._stats_lock:
                        self.stats["variation_requests"] += n_varied
            finally:
                self._leave_style()
        t2 = _t.perf_counter()
        if self.timing is not None:                  # LCM_WORKER_TIMING=1: (batch, conditioning s, sampler call s, end time)
            self.timing.append((len(items), t1 - t0, t2 - t1, t2))
        return res

    def _run_refine(self, pipe, key, items, noises, pe, kw, lane, stream, var_kw=lambda idx: {}):
        """The passes of a refinement batch (key = plain key + (d, p)).  Every item starts from its deepest cached x^k, k < p;
        items of one sampler pass must share that depth, so the batch is split by it (and each part cut to the plan batch
        sizes).  Every x^k a pass produces goes into the cache.  The bytes never depend on where a chain started: the draws of
        the passes left out are skipped, and the re-noise launch gives the bits of the hand-over step."""
        width, height, steps, g = key[:4]
        d, p = key[6], key[7]
        cache = self.refine_cache
        # (a varied request's x^k are its own: the resolved variation is part of the identity)
        idents = [_refine.request_ident(it[0], key, it[1], getattr(it, "ident", None)) for it in items]
        found = [cache.deepest(idn, d, p) if cache.cap > 0 else (None, None) for idn in idents]
        res = [None] * len(items)
        for k0, idx in _refine.group_by_start([f[0] for f in found], self.batch_sizes):
            with torch.cuda.stream(stream):          # the rows are gathered on the lane's stream, behind the text encoder
                sub_pe, sub_kw = _rows((pe, kw), idx, len(items))
            start = None if k0 is None else (k0, [found[i][1] for i in idx])
            out = pipe.generate(sub_pe, [items[i][1] for i in idx], width, height, steps, g,
                                noises=[noises[i] for i in idx] if noises is not None else None, lane=lane,
                                strength=d, passes=p, start=start, **var_kw(idx), **sub_kw)
            puts = 0
            if cache.cap > 0:
                first = out["xk_first"]
                with torch.cuda.stream(stream):
                    for j in range(0 if k0 is None else 1, out["xk"].shape[0]):
                        for b, i in enumerate(idx):
                            ck = idents[i] + (d, first + j)
                            if ck not in cache:      # a repeated (padding) item, or a depth another lane just filled
                                puts += bool(cache.put(ck, out["xk"][j, b].clone()))
                stream.synchronize()                 # the copies have landed before another lane may read them
            with self._stats_lock:
                self.stats["unet_evals"] += out["unet_evals"]
                self.stats["refine_cache_hits"] += len(idx) if k0 is not None else 0
                self.stats["refine_cache_misses"] += len(idx) if k0 is None else 0
                self.stats["refine_cache_puts"] += puts
            _take(res, out, idx)
        return res

    def _run_sdupscale(self, pipe, item, i, n, pe, kw, cap, lane, stream, shape, smp_kw):
        """One SD-upscale job (item ``i`` of the ``n`` the conditioning was encoded for): its T tiles in row-major order as
        image-to-image passes of the largest plan size that fits both the tiles left and ``cap`` (tile k: seed + k, its own draws,
        the request's conditioning row repeated), every pass's decoded pictures kept in the lane's tile store; then one combine
        launch and one read-back of the W x H picture.  -> (rgb [H, W, 3], the pool8 row of tile 0).  ``unet_evals`` counts every
        tile's evaluations."""
        tile_w, tile_h, steps, strength, g = shape
        req, seed, draws, pics, grid = item
        T = len(pics)
        seeds = _sdupscale.tile_seeds(seed, T)
        store = pipe.grid_store(lane, T, tile_h, tile_w)
        pool8, evals, k0 = None, 0, 0
        for m in _sdupscale.pass_sizes(T, cap, self.batch_sizes):
            with torch.cuda.stream(stream):          # the request's row, once per slot, behind the text encoder
                sub_pe, sub_kw = _rows((pe, kw), [i] * m, n)
            out = pipe.generate_img2img(sub_pe, seeds[k0:k0 + m], _fit.stack(pics[k0:k0 + m]), tile_w, tile_h, steps, strength, g,
                                        noises=draws[k0:k0 + m] if draws is not None else None, lane=lane, tiles=(store, k0, m),
                                        **smp_kw, **sub_kw)
            if pool8 is None:
                pool8 = out["pool8"][0:1]
            evals += out["unet_evals"] * m
            k0 += m
        rgb = pipe.combine_grid(lane, store, grid.W, grid.H, grid.overlap, grid.xs, grid.ys)
        with self._stats_lock:
            self.stats["unet_evals"] += evals
            self.stats["sdupscale_requests"] += 1
            self.stats["sdupscale_tiles"] += T
            self.stats["resized_on_device"] += int(any(_fit.is_pending(p) for p in pics))
        return rgb, pool8

    def _run_capped(self, items, noises, pe, kw, cap, stream, stat, call):
        """A hires, image-to-image or inpaint batch as passes of at most ``cap`` items (the largest plan size whose split-K workspace
        need fits the lane -- the pipeline's hires_batch_cap / img2img_batch_cap: a request never fails on workspace a smaller
        pass would have served; bit-neutral, a request's bytes do not depend on its batch).  call(idx, sub_pe, sub_noises,
        sub_kw) -> the pipeline's result dict for the items ``idx``; stat: the requests counter of the kind.
        -> per-item (rgb, pool8 row)."""
        n = len(items)
        res = [None] * n
        evals = 0
        for i0 in range(0, n, min(cap, n)):
            idx = list(range(i0, min(n, i0 + cap)))
            if len(idx) not in self.batch_sizes:     # a tail that is no plan size: its last item repeated (results dropped)
                idx += [idx[-1]] * (min(s for s in self.batch_sizes if s >= len(idx)) - len(idx))
            with torch.cuda.stream(stream):          # the rows are gathered on the lane's stream, behind the text encoder
                sub_pe, sub_kw = _rows((pe, kw), idx, n)
            out = call(idx, sub_pe, [noises[i] for i in idx] if noises is not None else None, sub_kw)
            evals += out["unet_evals"]
            _take(res, out, idx)
        with self._stats_lock:
            self.stats["unet_evals"] += evals
            self.stats[stat] += len({id(it) for it in items})
        return res

    def start_batcher(self):
        mb = int(os.environ.get("LCM_MICROBATCH", "8") or 0)
        if mb <= 1 and self.n_lanes <= 1:
            return
        from .batching import MicroBatcher
        ref = weakref.ref(self)

        def dispatch(key, items, lane=0):            # the dispatcher threads must not keep the engine alive
            eng = ref()
            if eng is None:
                raise RuntimeError("worker engine is gone")
            return eng.run_batch(key, items, lane)
        self.batcher = MicroBatcher(dispatch, max_batch=max(mb, 1), window_ms=float(os.environ.get("LCM_MICROBATCH_WINDOW_MS", "0") or 0),
                                    lanes=self.n_lanes)
        self.batch_sizes = tuple(self.batcher.sizes)
        weakref.finalize(self, self.batcher.close)   # engine collected without close(): stop the dispatcher threads

    def release(self) -> bool:
        """One worker less; the last one out shuts the engine down.  -> True when it did."""
        with _ENGINES_LOCK:
            self.refs -= 1
            if self.refs > 0:
                return False
            for k in [k for k, v in _ENGINES.items() if v() is self or v() is None]:
                del _ENGINES[k]
        self.shutdown()
        return True

    def shutdown(self):
        b, self.batcher = self.batcher, None
        if b is not None:
            b.close()
        for lk in self.lane_locks:
            lk.acquire()
        try:
            pipe, self.pipe = self.pipe, None
            if pipe is not None:
                pipe.close()                          # graphs dropped, split-K workspaces unregistered
            self.encode, self.enc, self.tok, self.styles, self.active_style = None, [], [], {}, None
            self.lane_encoders = {}
            self.refine_cache.clear()
        finally:
            for lk in self.lane_locks:
                lk.release()


_DEFAULT_CHUNKER = None


def _default_prompt_ctx(req, guidance):
    """Chunk count of a request for ``HipLcmWorker._job_key`` called without a worker: the synthetic runs' tokenizer."""
    global _DEFAULT_CHUNKER
    if _DEFAULT_CHUNKER is None:
        from ..clip import HashTokenizer
        _DEFAULT_CHUNKER = _prompt.PromptChunker(HashTokenizer())
    return _DEFAULT_CHUNKER.count(getattr(req, "prompt", ""))


_ENGINES: dict = {}              # key -> weakref.ref(_Engine)
_ENGINES_LOCK = threading.Lock()


class HipLcmWorker:
    """SD1.5-family worker (drop-in for DiffusersCudaWorker, backends/cuda_worker.py:20-304)."""

    FAMILY = "sd15"
    CONTROLNET_OK = True
    IMG2IMG_OK = True

    def __init__(self, worker_id: int, controlnet: str = None):
        """controlnet: a diffusers ControlNet directory or .safetensors file ("synthetic" with MODEL=synthetic*); None: the
        CONTROLNET environment variable.  Loaded on the first request that carries ``controlnet_image``."""
        self.worker_id = worker_id
        cn_src = (controlnet if controlnet is not None else os.environ.get("CONTROLNET") or "").strip() or None
        self._engine = None
        model_root = (os.environ.get("MODEL_ROOT") or "").strip()
        model_name = (os.environ.get("MODEL") or "").strip()
        synthetic = model_name.startswith("synthetic") or os.environ.get("LCM_HIP_SYNTHETIC", "0").lower() in ("1", "true", "yes", "on")
        if not synthetic:
            if not model_root:
                raise RuntimeError("MODEL_ROOT is required for BACKEND=hip")
            if not model_name:
                raise RuntimeError("MODEL is required for BACKEND=hip")
        _sampler.mode()                              # LCM_SAMPLERS: its own error, before anything is loaded
        dtype_str = os.environ.get("CUDA_DTYPE", "fp16").lower().strip()
        if dtype_str not in ("fp16", "bf16", "fp32"):
            raise RuntimeError(f"Unknown CUDA_DTYPE={dtype_str}, expected fp16, bf16 or fp32")      # cuda_worker.py:55-61
        if dtype_str != "fp16" and os.environ.get("LCM_HIP_DTYPE", "").lower().strip() != "fp16":
            # The reference honours bf16 / fp32 (torch dtype of the whole pipeline, cuda_worker.py:55-61).  This backend has ONE
            # arithmetic: fp16 operands, fp32 accumulation, fp32 sampler state -- inside north_star's tolerance of the fp32 pipeline
            # (max |delta| < 1e-2 on the decoded image; measured ~2e-3), but not what the setting asks for.  So it is refused,
            # not silently reinterpreted; LCM_HIP_DTYPE=fp16 states the override explicitly.
            raise RuntimeError(f"CUDA_DTYPE={dtype_str} is not available with BACKEND=hip: the HIP kernels compute with fp16 operands and "
                               f"fp32 accumulation only.  Set CUDA_DTYPE=fp16, or LCM_HIP_DTYPE=fp16 to run this mode in that arithmetic "
                               f"(max |delta| vs the fp32 pipeline < 1e-2 on the decoded image)")
        if not torch.cuda.is_available():
            raise LcmHipError("HipLcmWorker needs an MI355X; no CPU fallback exists on this path")
        from .worker_factory import pick_device
        device = pick_device(worker_id, torch.cuda.device_count())      # LCM_DEVICES=all: worker i -> GPU i mod N
        share = os.environ.get("LCM_SHARE_ENGINE", "1").lower() not in ("0", "false", "no", "off")
        from .styles import STYLE_REGISTRY
        # synthetic weights: the engine is keyed by the synthetic model's name (synthetic / synthetic-sd2 differ)
        synth_name = model_name if model_name.startswith("synthetic") else "synthetic"
        ekey = (self.FAMILY, device, synth_name if synthetic else os.path.join(model_root, model_name),
                tuple(sorted((sid, sd.path()) for sid, sd in STYLE_REGISTRY.items())), cn_src)
        with _ENGINES_LOCK:
            ref = _ENGINES.get(ekey) if share else None
            eng = ref() if ref is not None else None
            if eng is not None and eng.pipe is not None:
                eng.refs += 1
            else:
                eng = None
        if eng is not None:                          # a sibling worker already holds this checkpoint on this GPU
            self._engine = eng
            self._bind_prompt_ctx()
            print(f"[hip] worker {worker_id} ({self.FAMILY}) attached to the resident engine on {device} ({eng.refs} workers)")
            return
        sched = LCMSchedule()
        clip_sd = text_cfg = None
        if synthetic and synth_name == "synthetic-sd2" and self.FAMILY == "sd15":
            from ..clip import CLIP_H
            from ..config import SD2_UNET, unet_config
            from ..scheduler import SD21_768_SCHEDULE
            usd, ucfg, vsd, vcfg = _weights.synthetic_sd2_unet(), unet_config(SD2_UNET), _weights.synthetic_vae(), None
            sched, text_cfg = LCMSchedule(**SD21_768_SCHEDULE), dict(CLIP_H)
            ckpt_root, ckpt, format_name = None, synth_name, "synthetic"
        elif synthetic:
            usd, ucfg, vsd, vcfg = self._synthetic_weights()
            ckpt_root, ckpt, format_name = None, "synthetic", "synthetic"
        else:
            ckpt = os.path.join(model_root, model_name)
            if os.path.isdir(ckpt) and os.path.exists(os.path.join(ckpt, "model_index.json")):
                usd, ucfg, vsd, vcfg = _weights.load_diffusers_dir(ckpt)          # cuda_worker.py:66-77
                sched = LCMSchedule.from_config_file(os.path.join(ckpt, "scheduler", "scheduler_config.json"))
                format_name = "diffusers"
            elif os.path.isfile(ckpt) and ckpt.endswith(".safetensors"):
                # a file has no scheduler/ folder: the loader says what its UNet predicts (LCM_PREDICTION_TYPE overrides)
                if self.FAMILY == "sd15":
                    usd, ucfg, vsd, vcfg, clip_sd, meta = _weights.load_single_file(ckpt, with_meta=True)   # cuda_worker.py:78-85
                    pred, text_cfg = meta["prediction_type"], meta["text_config"]
                else:
                    usd, ucfg, vsd, vcfg, clip_sd = _weights.load_single_file_sdxl(ckpt)                   # cuda_worker.py:330-352
                    pred = _weights.single_file_prediction_type({}, False)
                sched = LCMSchedule(prediction_type=pred)
                format_name = "single-file"
            else:
                raise RuntimeError(f"{ckpt}: expected a diffusers directory (model_index.json) or a .safetensors file"
                                   " (.ckpt pickles are not loaded: they execute code)")
            cad = int(ucfg.get("cross_attention_dim", 768))
            if (cad in (2048, 1280)) != (self.FAMILY == "sdxl"):
                raise RuntimeError(f"Loaded UNet with cross_attention_dim={cad} into the {self.FAMILY} worker "
                                   "(SD1.5: 768/1024, SDXL: 2048)")                  # cuda_worker.py:114-116
            ckpt_root = ckpt if format_name == "diffusers" else None
        if self.FAMILY == "sd15" and vcfg is not None:
            # only the SDXL pipeline honours the VAE's force_upcast (StableDiffusionXLPipeline.upcast_vae); SD1.5 decodes in
            # the pipeline dtype whatever the checkpoint's vae/config.json says
            vcfg = dict(vcfg, force_upcast=False, residual_scale=1.0)
        eng = _Engine(type(self))
        eng.device = device
        eng.pipe = LcmHipPipeline(usd, vsd, ucfg, vcfg, device=device, schedule=sched)
        if self.IMG2IMG_OK:
            # the VAE encoder of image-to-image: where it comes from, nothing uploaded until a request carries a picture
            # (synthetic weights are not even generated before that)
            eng.pipe.set_vae_encoder_source(_weights.synthetic_vae_encoder if synthetic else getattr(vsd, "encoder", None), vcfg)
        with torch.cuda.stream(eng.pipe.stream):
            self._load_text_encoders(eng, device, ckpt_root, clip_sd, text_cfg)
        eng.refs = 1
        eng.controlnet_src, eng.synthetic_model = cn_src, bool(synthetic)
        self._engine = eng
        self._bind_prompt_ctx()
        self._load_styles(eng)
        eng.start_batcher()
        if share:
            with _ENGINES_LOCK:
                _ENGINES[ekey] = weakref.ref(eng)
        print(f"[hip] worker {worker_id} ({self.FAMILY}) loaded: {os.path.basename(ckpt)} ({format_name}) on {device} dtype=fp16 "
              f"unet={eng.pipe.unet.weight_bytes() / 1e9:.2f}GB vae={eng.pipe.vae.weight_bytes() / 1e9:.2f}GB "
              f"text={self._text_bytes(eng) / 1e9:.2f}GB")

    # ---- the reference's attributes (tests/test_sdxl_worker.py:118-130), served from the shared engine --------------
    @property
    def pipe(self):
        return self._engine.pipe if self._engine is not None else None

    @property
    def device(self):
        return self._engine.device if self._engine is not None else None

    @property
    def dtype(self):
        return torch.float16

    @property
    def _styles(self):
        return self._engine.styles if self._engine is not None else {}

    @property
    def _active_style(self):
        return self._engine.active_style

    # ---- style LoRAs (backends/cuda_worker.py:123-196) -----------------------------------------
    @classmethod
    def _load_styles(cls, eng):
        from ..lora import StyleAdapters
        from .styles import STYLE_REGISTRY
        cad = int(eng.pipe.unet.ctx_dim)
        for sid, sd in STYLE_REGISTRY.items():
            if sd.required_cross_attention_dim is not None and int(sd.required_cross_attention_dim) != cad:
                print(f"[hip] skip style '{sid}': incompatible cross_attention_dim (model={cad} style={sd.required_cross_attention_dim})")
                continue
            path = sd.path()
            if not os.path.exists(path):
                print(f"[hip] style '{sid}': LoRA file {path} not found; style disabled")
                continue
            try:
                from safetensors.torch import load_file
                with torch.cuda.stream(eng.pipe.stream):
                    st = StyleAdapters(eng.pipe.unet, cls._text_encoders(eng), load_file(path))
                eng.styles[sid] = st
                print(f"[hip] loaded style LoRA: {sid} -> {path} ({len(st.modules)} UNet + {st.text_modules} text-encoder modules, "
                      f"{len(st.skipped)} tensors skipped, {st.nbytes() / 1e6:.0f} MB)")
            except Exception as e:
                print(f"[hip] FAILED to load style LoRA {sid}: {e!r}")

    def _apply_style(self, style_id, level):
        """The reference's hook (backends/cuda_worker.py:149-196).  The merged weights are shared by every lane, so -- like
        ``_enter_style`` -- the re-merge waits until no pass is in flight: weights are never rewritten under a running graph."""
        eng = self._engine
        with eng._style_cv:
            while eng._style_users > 0 and eng._want_style(style_id, level) != eng.active_style:
                eng._style_cv.wait()
            eng.apply_style(style_id, level)

    # ---- family hooks (operate on the engine: no worker object is ever captured by shared state) ----------------------
    def _synthetic_weights(self):
        return _weights.synthetic_unet(), None, _weights.synthetic_vae(), None

    @staticmethod
    def _load_text_encoders(eng, device, ckpt_root, clip_sd, text_cfg=None):
        # CLIP text encoder on the same kernels (checkpoint text_encoder/ when present, else synthetic weights: CLIP-L, or
        # text_cfg's tower -- CLIP-H for synthetic-sd2)
        eng.encode = HipPromptEncoder(device, ckpt_root, clip_sd, text_cfg)
        if eng.encode.enc.D != eng.pipe.unet.ctx_dim:
            raise RuntimeError(f"text encoder width {eng.encode.enc.D} != UNet cross_attention_dim {eng.pipe.unet.ctx_dim}")

    @staticmethod
    def _text_encoders(eng):
        return [eng.encode.enc]

    @staticmethod
    def _text_bytes(eng):
        return eng.encode.enc.weight_bytes()

    @staticmethod
    def _conditioning(eng, reqs, width, height, guidance, lane=0, n_ctx=1):
        """-> (prompt_embeds [B,77 n,ctx], kwargs for LcmHipPipeline.generate) for B requests of one batch, n = n_ctx chunks each
        (backends/prompt_syntax.py).  Under classifier-free guidance the requests' negative prompts are the unconditional half, and
        the shorter of (prompt, negative prompt) is filled with empty-prompt chunks to n (A1111 with ``pad_cond_uncond`` on; its
        default runs the two halves unpadded).  Every chunk of the pass goes through CLIP in one batch."""
        B = len(reqs)
        encode, _ = eng._lane_encoders(lane)
        ck, L = encode.chunker, encode.enc.L
        do_cfg = guidance > 1.0 and not eng.pipe.unet.has_cond

        def fill(c):                                 # (the cached Chunked is never touched)
            if c.n == n_ctx:
                return c
            if c.n > n_ctx:
                raise RuntimeError(f"a prompt of {c.n} chunks in a pass of {n_ctx}")
            e_ids, e_w = ck.empty_chunk()
            return _prompt.Chunked(c.ids + [e_ids] * (n_ctx - c.n), c.weights + [e_w] * (n_ctx - c.n), c.n_tokens)
        texts = [fill(ck.chunk(r.prompt)) for r in reqs]
        stops = [L - (_prompt.parse_clip_skip(r, L) - 1) for r in reqs]
        weighted = sum(t.weighted for t in texts)
        if do_cfg:
            negs = [fill(ck.chunk(_prompt.negative_text(r))) for r in reqs]
            weighted += sum(n.weighted and not t.weighted for n, t in zip(negs, texts))
            if n_ctx == 1 and len(set(stops)) == 1 and not any(n.ids != negs[0].ids or n.weighted for n in negs):
                # one unconditional row serves the batch (all of them are the same text, usually ""): encoded once
                pe, n1 = encode.encode_chunked(texts, stops)
                neg, n2 = encode.encode_chunked(negs[:1], stops[:1])
                neg = neg.expand(B, -1, -1)
            else:
                both, n1 = encode.encode_chunked(negs + texts, stops + stops)
                neg, pe, n2 = both[:B], both[B:], 0
        else:
            (pe, n1), neg, n2 = encode.encode_chunked(texts, stops), None, 0
        with eng._stats_lock:
            eng.stats["prompt_chunks"] += n1 + n2
            eng.stats["weighted_prompts"] += weighted
        return pe, dict(negative_embeds=neg)

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _job_key(req, prompt_ctx=None):
        """What must agree for jobs to share one batched pass: geometry, step count, guidance and style merge -- and, for a
        refinement request (``denoise_strength`` / ``pass_number``, backends/refine.py), its strength and pass number: those
        get a key of their own (the plain fields plus (d, p)) and never share a pass with plain requests.  Hires requests
        (``enable_hr``, backends/hires.py) coalesce among themselves: the plain key + ("hires", target size, hr_steps, strength,
        mode).  Image-to-image requests (a picture, backends/img2img.py) get the plain key + ("img2img", strength); with a mask
        (backends/inpaint.py) they are inpaint requests with the plain key + ("inpaint", strength, mask_blur) instead.
        A request with a served ``sampler_name`` (backends/sampler.py; plain, ControlNet and image-to-image requests) appends
        ("sampler", canonical name, "karras" | "normal") to its kind's key: such jobs coalesce among themselves.
        An SD-upscale request (``script_name``, backends/sdupscale.py) appends ("sdupscale", overlap, upscaler, W, H) to its
        image-to-image key: such jobs may be drained together, then run one after the other -- tiles of two requests never share a pass.
        A prompt of n > 1 chunks (backends/prompt_syntax.py; under classifier-free guidance the longer of prompt and negative
        prompt counts) appends ("ctx", n) to whichever of these keys the request has: the pass has 77 n context rows.  With n == 1 --
        weighted or not, with or without a negative prompt -- the key is the one of always; the texts and ``clip_skip`` are per
        image.  prompt_ctx(req, guidance) -> n: the engine's chunk count (a worker binds its own tokenizer, ``_bind_prompt_ctx``);
        None: counted with the synthetic runs' stand-in tokenizer and no classifier-free guidance."""
        key = HipLcmWorker._kind_key(req)
        n = (prompt_ctx or _default_prompt_ctx)(req, key[3])
        return key if n <= 1 else key + (_prompt.CTX_TAG, n)

    @staticmethod
    def _kind_key(req):
        width, height = parse_size(req.size)
        sl = getattr(req, "style_lora", None)
        style_id = getattr(sl, "style", None) if sl else None
        level = int(getattr(sl, "level", 0) or 0) if sl else 0
        if not style_id or level <= 0:
            style_id, level = None, 0
        key = (width, height, int(req.num_inference_steps), float(req.guidance_scale), style_id, level)
        rf = _refine.parse_refine(req)
        ctl = _controlnet.parse_control(req)
        hr = _hires.parse_hires(req, width, height, key[2])
        i2i = _img2img.parse_img2img(req)
        inp = _inpaint.parse_inpaint(req)            # a mask without a picture raises here
        if i2i is not None:
            _fit.parse_resize_mode(req)              # its own error, for its own job; no part of the key (the picture is per image)
        # SD upscale (``script_name``, backends/sdupscale.py): None for every request without the script -- today's key
        sdu = _sdupscale.parse_sdupscale(req, i2i, width, height)
        if sdu is not None and inp is not None:
            raise RuntimeError(_sdupscale.NOT_COMBINED + "mask")
        # variation seeds / seed-resize (backends/variation.py): their own errors, for their own job; no part of the key -- the
        # variation is per image, plain and varied requests share passes
        if _variation.parse_variation(req, width, height) is not None and (i2i is not None or inp is not None):
            raise RuntimeError(_variation.NOT_COMBINED)
        smp = _sampler.parse_sampler(req)            # None: the LCM sampler, the key of always
        if smp is not None:
            if inp is not None:
                raise RuntimeError(_sampler.NOT_COMBINED + "mask")
            if hr is not None:
                raise RuntimeError(_sampler.NOT_COMBINED + "enable_hr")
            if rf is not None:
                raise RuntimeError(_sampler.NOT_COMBINED + "refinement (denoise_strength < 1 or pass_number > 1)")
        tail = _sampler.tail(smp)
        if inp is not None:
            # inpaint jobs coalesce among themselves, never with image-to-image jobs: the plain key + strength and mask blur
            if hr is not None:
                raise RuntimeError("mask is not combined with enable_hr")
            if rf is not None:
                raise RuntimeError("mask is not combined with refinement (denoise_strength < 1 or pass_number > 1)")
            if ctl is not None:
                raise RuntimeError("mask is not combined with controlnet_image")
            return key + (_inpaint.KEY_TAG, inp[0], inp[1])
        if i2i is not None:
            # image-to-image jobs coalesce among themselves: the plain key + the strength (the picture is per image)
            if hr is not None:
                raise RuntimeError("init_image is not combined with enable_hr")
            if rf is not None:
                raise RuntimeError("init_image is not combined with refinement (denoise_strength < 1 or pass_number > 1)")
            if ctl is not None:
                raise RuntimeError("init_image is not combined with controlnet_image")
            # SD-upscale jobs: the image-to-image key + ("sdupscale", overlap, upscaler, W, H) -- never a pass with image-to-image
            # jobs; W x H come from the parse (they depend on the picture)
            return key + (_img2img.KEY_TAG, i2i[0]) + tail + _sdupscale.tail(sdu)
        if hr is not None:
            if rf is not None:
                raise RuntimeError("enable_hr is not combined with refinement (denoise_strength < 1 or pass_number > 1)")
            if ctl is not None:
                raise RuntimeError("enable_hr is not combined with controlnet_image")
            return key + (_hires.KEY_TAG,) + hr
        if ctl is not None:
            # ControlNet jobs coalesce among themselves: the plain key + the conditioning scale (the hint is per image) and,
            # with a preprocessor, its name and parameters: ("canny", lo, hi) / ("invert",)
            if rf is not None:
                raise RuntimeError("controlnet_image is not combined with refinement (denoise_strength < 1 or pass_number > 1)")
            return key + (_controlnet.KEY_TAG, ctl[0]) + _controlnet.parse_preprocessor(req) + tail
        return key + tail if rf is None else key + rf

    def _bind_prompt_ctx(self):
        """Give this worker's ``_job_key`` the engine's own chunk count: its tokenizer, its text encoder's depth (clip_skip is
        checked there, for its own job) and whether guidance above 1 means a negative prompt is encoded."""
        eng = self._engine
        if eng.encode is None:                       # SDXL: two encoders, prompts truncated to 77 tokens as ever
            return
        ck, L, cfg_capable = eng.encode.chunker, eng.encode.enc.L, not eng.pipe.unet.has_cond
        base = HipLcmWorker.__dict__["_job_key"].__func__

        def prompt_ctx(req, guidance):
            _prompt.parse_clip_skip(req, L)
            n = ck.count(getattr(req, "prompt", ""))
            if cfg_capable and guidance > 1.0:
                n = max(n, ck.count(_prompt.negative_text(req)))
            return n
        self._job_key = lambda req: base(req, prompt_ctx)

    def _run_batch(self, key, items):
        return self._engine.run_batch(key, items)

    @staticmethod
    def _drawable(key, *more) -> bool:
        """Can the request's noise be drawn ahead?  Its sizes are positive multiples of 8 and it has a step; anything else is
        left to the pipeline's own error."""
        return all(v % 8 == 0 and v > 0 for v in key[:2] + more) and key[2] >= 1

    def _prepare(self, req, key):
        """-> the request's item for ``run_batch``: ``_prepare_kind``'s tuple, as it is for every request without an active
        variation; with one, the same tuple as a ``variation.VariedItem`` that also carries the variation's draws."""
        return self._with_variation(self._prepare_kind(req, key), key)

    def _with_variation(self, item, key):
        """Variation seeds / seed-resize of the item's request (backends/variation.py): the subseed is resolved (a random one by
        the seed's own policy when none or -1 was sent; it is not reported: ``run_job`` has no place for it) and the variation's
        tensors are drawn HERE, on the caller's thread, from generators of their own (pipeline.py's RNG contract).  The
        request's own draws are untouched."""
        req, seed = item[0], item[1]
        var = _variation.parse_variation(req, key[0], key[1])
        if var is None:
            return item
        sub, t, hs, ws = var                         # (never on the SDXL worker: its _job_key has refused the request)
        resized = (hs, ws) != (key[1] // 8, key[0] // 8)
        subseed = _variation.resolve_subseed(sub) if t > 0.0 else None
        if not self._drawable(key):                  # left to the pipeline's own size error
            return item
        s, base = draw_variation_sources(seed, subseed, hs, ws, self._engine.pipe.sched.init_noise_sigma, resized=resized)
        return _variation.attach(item, (t, s, base), (subseed, t, hs, ws))

    def _prepare_kind(self, req, key):
        """-> (req, seed, noise[, hint | picture[, mask]]): the seed policy of cuda_worker.py:210-213 and the request's RNG stream.
        An upload that does not have the request's size is fitted here on the host (LCM_RESIZE=pil, or outside the device path's
        domain) or handed on at its own size as a ``fit.Pending`` for the lane's stream to fit (backends/fit.py)."""
        eng = self._engine
        key, _ = _prompt.split_ctx(key)              # the prompt's length changes nothing here
        key, sdu = _sdupscale.split_key(key)
        key, smp = _sampler.split_key(key)           # a sampler draws exactly what the LCM sampler draws for the request
        seed = int(req.seed) if getattr(req, "seed", None) is not None else int(torch.randint(0, 100_000_000, (1,)).item())
        # the request's RNG stream (initial latents, then one draw per remaining step) is drawn HERE, on the caller's
        # thread: pool threads do it in parallel and the GPU dispatcher's serial path shrinks by ~0.5 ms per request
        sched = eng.pipe.sched
        h8, w8, steps = key[1] // 8, key[0] // 8, key[2]
        n_draws, more = steps, ()
        if _inpaint.is_inpaint_key(key):             # as image-to-image (the same draws), plus the fitted mask
            eng.ensure_vae_encoder()
            _refine.check_schedule(sched, steps, key[7])
            _, _, pic, mask = _inpaint.parse_inpaint(req)
            mode = _fit.parse_resize_mode(req)       # picture and mask alike, as in A1111
            return (req, seed, draw_noise_img2img(seed, h8, w8, steps) if self._drawable(key) else None,
                    _fit.prepare(pic, key[0], key[1], mode, _img2img.fit_init), _fit.prepare(mask, key[0], key[1], mode, _inpaint.fit_mask))
        if _img2img.is_img2img_key(key):             # encoder on first use, the schedule's own error, the picture, the draws
            eng.ensure_vae_encoder()
            if smp is None:
                _refine.check_schedule(sched, steps, key[7])
            else:                                    # the LCM-only step bound does not apply; DDIM with no timestep left raises here
                _sampler.check_img2img(sched, smp, steps, key[7])
            if sdu is not None:
                # SD upscale: tile k is the image-to-image request of its own pixels with seed + k -- its draws are that
                # request's, its picture a window of the one resample grid (resize_mode is not applied: nothing is fitted to size)
                _, _, _, _, g = _sdupscale.parse_sdupscale(req, _img2img.parse_img2img(req), key[0], key[1])
                pics, _ = _sdupscale.tile_pictures(_img2img.parse_img2img(req)[1], g)
                draws = ([draw_noise_img2img(s, h8, w8, steps) for s in _sdupscale.tile_seeds(seed, len(pics))]
                         if self._drawable(key) else None)
                return (req, seed, draws, pics, g)
            pic = _fit.prepare(_img2img.parse_img2img(req)[1], key[0], key[1], _fit.parse_resize_mode(req), _img2img.fit_init)
            return (req, seed, draw_noise_img2img(seed, h8, w8, steps) if self._drawable(key) else None, pic)
        if _hires.is_hires_key(key):                 # the schedule's own error first, then the draws at both shapes
            tw, th, hr_steps, strength = key[7:11]
            _refine.check_schedule(sched, hr_steps, strength)
            return (req, seed, draw_noise_hires(seed, h8, w8, steps, th // 8, tw // 8, hr_steps, sched.init_noise_sigma)
                    if self._drawable(key, tw, th) else None)
        if _controlnet.is_control_key(key):
            eng.ensure_controlnet()                  # lazily, on the caller's thread; raises for this job
            more = (_fit.prepare(_controlnet.parse_control(req)[1], key[0], key[1], _fit.JUST_RESIZE, _controlnet.fit_hint),)
        elif len(key) > 6:                           # refinement: the schedule's own error first, then the whole chain's draws
            _refine.check_schedule(sched, steps, key[6])
            n_draws = _refine.noise_draws(steps, key[7])
        noise = draw_noise(seed, h8, w8, n_draws - 1, sched.init_noise_sigma) if self._drawable(key) else None
        return (req, seed, noise) + more

    def _submit(self, job):
        eng = self._engine
        if eng is None or eng.pipe is None:
            raise RuntimeError("worker is closed")
        req = job.req
        key = self._job_key(req)                     # raises the reference's size error in the caller's thread
        item = self._prepare(req, key)
        b = eng.batcher
        if b is None:
            return eng.run_batch(key, [item])[0], item[1]
        return b.submit(key, item).result(), item[1]

    # ---- batching behind the reference's single-consumer pool ------------------------------------------
    def bind_queue(self, q) -> None:
        """Tell the worker which ``queue.Queue`` its caller's consumer thread takes jobs from (``WorkerPool.q``,
        backends/worker_pool.py:171).  Not needed behind ``get_worker_pool()``: that singleton is found by itself."""
        self._pool_q = q

    def _pool_queue(self):
        q = getattr(self, "_pool_q", None)
        if q is not None:
            return q
        if os.environ.get("LCM_DRAIN_QUEUE", "1").lower() in ("0", "false", "no", "off"):
            return None
        # the reference's process-wide pool (backends/worker_pool.py:421-469): looked up, never imported -- only when the
        # reference's module is already loaded and its pool is the one currently holding THIS worker
        import sys
        mod = sys.modules.get("backends.worker_pool")
        pool = getattr(mod, "_worker_pool", None) if mod is not None else None
        if pool is not None and getattr(pool, "_worker", None) is self:
            return getattr(pool, "q", None)
        return None

    def _drain(self, q, job, key, limit):
        """Take from the pool's queue, under its own mutex, the queued jobs that can share this call's sampler pass.

        ``WorkerPool._worker_loop`` is ONE thread that calls ``job.execute(worker)`` -> ``worker.run_job(job)`` and blocks
        (backends/worker_pool.py:294-341, :84-88): ``run_job`` never sees a second job, so the batch has to be collected
        here.  Rules: walk the queue from its head; a job qualifies when it is of the same class as the running one (the
        pool would have called ``run_job`` for it too), carries ``.req`` and an unresolved ``.fut``, and its request agrees on
        (size, steps, guidance, style); generation jobs with another key keep their place; the walk STOPS at the first
        job of any other kind (a ``ModeSwitchJob`` / ``CustomJob`` is a barrier: nothing queued behind it is overtaken).
        A drained job is finished here exactly as the loop would have (worker_pool.py:328-339): its future gets
        ``(png, seed)`` or the exception, and ``q.task_done()`` is called for it."""
        taken = []
        if limit <= 0:
            return taken
        cls = type(job)
        with q.mutex:
            dq = q.queue
            idx = []
            for i, j in enumerate(dq):
                if type(j) is not cls or not hasattr(j, "req") or getattr(j, "fut", None) is None:
                    break                             # barrier
                try:
                    same = (not j.fut.done()) and self._job_key(j.req) == key
                except Exception:
                    same = False                      # malformed request: it raises from its own run_job call, in its turn
                if same:
                    idx.append(i)
                    if len(idx) >= limit:
                        break
            for i in reversed(idx):
                taken.append(dq[i])
                del dq[i]
            if idx:
                q.not_full.notify(len(idx))           # space for blocked producers (Queue.put)
        taken.reverse()
        return taken

    def _finish_drained(self, q, job, fut, seed):
        """Runs on a finisher thread when the drained job's pass is done: what the pool's loop does for a job
        (backends/worker_pool.py:328-339)."""
        try:
            rgb, _ = fut.result()
            res = (encode_png(rgb), seed)
            if not job.fut.done():
                job.fut.set_result(res)
        except BaseException as e:                    # noqa
            try:
                if not job.fut.done():
                    job.fut.set_exception(e)
            except Exception:
                pass
        finally:
            q.task_done()

    def _gather_wait(self, q, want):
        """Closed-loop callers come back together: the clients of the previous call's batch get their results within a few
        milliseconds of each other and re-submit.  If that call drained k jobs, give about as many time to arrive before taking
        the batch -- otherwise the first arrival runs alone and the rest wait a whole pass for a small batch.  The window is a
        tenth of what the previous call took (a batched pass takes 35-125 ms), at most LCM_DRAIN_WINDOW_MS (default 12); a lone
        caller (k == 0) never waits."""
        import time as _t
        k = getattr(self, "_last_drained", 0)
        if k <= 0:
            return
        cap = float(os.environ.get("LCM_DRAIN_WINDOW_MS", "12") or 0) * 1e-3
        win = min(cap, max(0.002, 0.1 * getattr(self, "_last_call_s", 0.0)))
        if cap <= 0:
            return
        # ... but only while jobs keep coming: callers that come back together (closed loop) fill the queue within a millisecond,
        # a job every few hundred microseconds; under steady independent arrivals nothing comes for milliseconds and the wait is
        # pure added service time (open loop at 80 / 100 requests/s: p50 51 / 83 ms without it against 61 / 103 with).  So the
        # wait ends as soon as the queue has been still for 0.6 ms.  The target is one MORE job than last time: the previous
        # call's OWN caller gets its result last (the pool resolves that future after run_job returns,
        # backends/worker_pool.py:330-332) and re-submits a thread wake-up later -- taken without it, its job waits a whole pass
        # and then leads the next call, again one short: a stable state of 15 + 1 instead of 16.
        now = _t.perf_counter()
        deadline, last_n, last_t = now + win, q.qsize(), now
        while last_n < want(k + 1) and now < deadline:
            _t.sleep(0.0002)
            now = _t.perf_counter()
            n = q.qsize()
            if n != last_n:
                last_n, last_t = n, now
            elif now - last_t > 0.0006:
                break

    def run_job(self, job) -> Tuple[bytes, int]:
        eng = self._engine
        q = self._pool_queue() if eng is not None and getattr(eng, "batcher", None) is not None else None
        if q is None:
            (rgb, _), seed = self._submit(job)
            return encode_png(rgb), seed
        b = eng.batcher
        limit = b.max_batch * max(1, b.lanes) - 1
        import time as _t
        t_in = _t.perf_counter()
        self._gather_wait(q, lambda k: min(k, limit))
        t_call = _t.perf_counter()
        if q.empty():
            self._last_drained = 0
            (rgb, _), seed = self._submit(job)
            return encode_png(rgb), seed
        if eng.pipe is None:
            raise RuntimeError("worker is closed")
        key = self._job_key(job.req)
        # as many as the lanes can have in flight as full batches (two batch-8 passes on two lanes: 127 against 116 images/s)
        others = self._drain(q, job, key, limit)
        self._last_drained = len(others)
        if not others:
            (rgb, _), seed = self._submit(job)
            return encode_png(rgb), seed
        pending, fin = [], _finish_pool()
        try:
            items = list(fin.map(lambda j: self._prepare(j.req, key), [job] + others))
            t_prep = _t.perf_counter()
            futs = [b.submit(key, it, burst=True) for it in items]        # a complete set: the lanes split it at once
        except BaseException as e:                    # noqa  nothing was started: the drained jobs fail like the running one
            for j in others:
                if not j.fut.done():
                    j.fut.set_exception(e)
                q.task_done()
            raise
        for j, f, it in zip(others, futs[1:], items[1:]):
            done = threading.Event()
            pending.append(done)

            def _cb(f, j=j, seed=it[1], done=done):
                done.set()                            # the GPU side of this job is over
                fin.submit(self._finish_drained, q, j, f, seed)
            f.add_done_callback(_cb)
        try:
            rgb, _ = futs[0].result()
            t_gpu = _t.perf_counter()
            png = encode_png(rgb)
            if getattr(eng, "timing", None) is not None:      # LCM_WORKER_TIMING=1: ("call", jobs, gather s, drain + prepare s, pass s, PNG s)
                eng.timing.append(("call", len(items), t_call - t_in, t_prep - t_call, t_gpu - t_prep, _t.perf_counter() - t_gpu))
            return png, items[0][1]
        finally:
            # return to the pool's loop only when every pass this call started has left the GPU (a mode switch may be next in
            # the queue); the drained jobs' PNGs may still be deflating on the finisher threads -- no GPU state involved.
            # (Returning as soon as the call's own job is done, to keep the second lane fed, was measured at 8 / 16 / 24
            # closed-loop clients: 79 / 100 / 99 images/s against 86 / 98 / 102 -- the callers fall out of step and the batches
            # shrink; not kept.)
            for ev in pending:
                ev.wait()
            self._last_call_s = _t.perf_counter() - t_call

    def run_job_with_latents(self, job) -> Tuple[bytes, int, bytes]:
        # The reference re-runs the whole pipeline for the latents (cuda_worker.py:255-283); the sampler is
        # deterministic in the seed, so the same pass's final latents are identical and are pooled on device.
        (rgb, pool8), seed = self._submit(job)
        return encode_png(rgb), seed, pool8.tobytes(order="C")

    def run_jobs(self, jobs):
        """Batched convenience entry (not in the reference's protocol): jobs that agree on ``_job_key`` run as one pass
        (chunked to the plan batch sizes); PNGs are encoded on a small thread pool.  -> [(png, seed)] in job order."""
        from concurrent.futures import ThreadPoolExecutor
        seeds, groups = [], {}
        for i, job in enumerate(jobs):
            req = job.req
            seeds.append(int(req.seed) if getattr(req, "seed", None) is not None else int(torch.randint(0, 100_000_000, (1,)).item()))
            key = self._job_key(req)
            if _img2img.is_img2img_key(key) or _inpaint.is_inpaint_key(key) or _controlnet.is_control_key(key):
                # these kinds (SD-upscale keys are image-to-image keys) carry an upload per item, which only ``_prepare`` builds
                raise RuntimeError("run_jobs does not serve requests with an upload (init_image, mask, controlnet_image, SD upscale): "
                                   "use run_job")
            groups.setdefault(key, []).append(i)
        rgbs = [None] * len(jobs)
        sizes = self._engine.batch_sizes
        for key, idx in groups.items():
            while idx:
                n = max(s for s in sizes if s <= len(idx))
                part, idx = idx[:n], idx[n:]
                items = [self._with_variation((jobs[i].req, seeds[i]), key) for i in part]
                for i, (rgb, _) in zip(part, self._engine.run_batch(key, items)):
                    rgbs[i] = rgb
        with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
            pngs = list(ex.map(encode_png, rgbs))
        return list(zip(pngs, seeds))

    def close(self):
        """Optional (the reference's pool never calls it): detach from the engine now instead of at garbage collection."""
        eng, self._engine = getattr(self, "_engine", None), None
        if eng is not None:
            eng.release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipLcmSDXLWorker(HipLcmWorker):
    CONTROLNET_OK = False        # a hint sent here raises for its job (SDXL ControlNets are out of scope)
    IMG2IMG_OK = False           # so does a picture: the SDXL VAE's encoder is out of scope
    """SDXL worker (drop-in for DiffusersSDXLCudaWorker, backends/cuda_worker.py:307-614): two text encoders
    (CLIP-L hidden_states[-2] | OpenCLIP-bigG hidden_states[-2] -> 2048; pooled bigG text_embeds), size/crop time ids,
    classifier-free guidance when guidance_scale > 1 (negative conditioning = zeros, force_zeros_for_empty_prompt)."""

    FAMILY = "sdxl"

    @staticmethod
    def _job_key(req):
        if _sdupscale.active(req):
            raise RuntimeError(_sdupscale.SDXL_ERROR)
        if getattr(req, "enable_hr", None):
            raise RuntimeError("enable_hr: hires fix is not served by the SDXL worker (SD1.5 and SD 2.x only)")
        if getattr(req, "init_image", None) is not None or getattr(req, "init_images", None) is not None:
            raise RuntimeError("init_image: image-to-image is not served by the SDXL worker (SD1.5 and SD 2.x only)")
        if getattr(req, "mask", None) is not None or getattr(req, "mask_image", None) is not None:
            raise RuntimeError("mask: inpainting is not served by the SDXL worker (SD1.5 and SD 2.x only)")
        if _variation.parse_variation(req, *parse_size(req.size)) is not None:
            raise RuntimeError(_variation.SDXL_ERROR)
        if _sampler.parse_sampler(req) is not None:
            raise RuntimeError(_sampler.SDXL_ERROR)
        return HipLcmWorker._kind_key(req)           # prompts are truncated to 77 tokens here, as ever: no ("ctx", n)

    def _synthetic_weights(self):
        from ..config import SDXL_UNET, unet_config, vae_config
        ucfg = unet_config(SDXL_UNET)
        vcfg = vae_config(dict(scaling_factor=0.13025, sample_size=1024, force_upcast=True))
        return (_weights.synthetic_state_dict(_weights.unet_param_spec(ucfg), 0), ucfg,
                _weights.synthetic_state_dict(_weights.vae_param_spec(vcfg), 1), vcfg)

    @staticmethod
    def _load_text_encoders(eng, device, ckpt_root, clip_sd, text_cfg=None):
        from ..clip import CLIP_BIGG, CLIP_L, ClipTextHip, HashTokenizer, load_clip_dir, synthetic_clip
        from ..prompt import make_tokenizer
        eng.enc, eng.tok = [], []
        for idx, (sub, tsub, cfg0, seed) in enumerate((("text_encoder", "tokenizer", CLIP_L, 2),
                                                       ("text_encoder_2", "tokenizer_2", CLIP_BIGG, 3))):
            d = os.path.join(ckpt_root, sub) if ckpt_root else None
            real = True
            if clip_sd is not None and clip_sd[idx] is not None:          # carried inside a single-file checkpoint
                sd = clip_sd[idx]
                D = sd["embeddings.token_embedding.weight"].shape[1]
                cfg = dict(cfg0, hidden_size=D, vocab_size=sd["embeddings.token_embedding.weight"].shape[0],
                           num_hidden_layers=1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers.")),
                           intermediate_size=sd["encoder.layers.0.mlp.fc1.weight"].shape[0], num_attention_heads=D // 64)
                if "text_projection.weight" in sd:
                    cfg["projection_dim"] = sd["text_projection.weight"].shape[0]
            elif d and os.path.isdir(d):
                sd, cfg = load_clip_dir(d)
                cfg = dict(cfg0, **cfg)
            else:
                sd, cfg, real = synthetic_clip(cfg0, seed=seed), cfg0, False
            eng.enc.append(ClipTextHip(sd, cfg, device=device))
            eng.tok.append(make_tokenizer(ckpt_root, tsub, cfg["vocab_size"], real))
        if eng.enc[0].D + eng.enc[1].D != eng.pipe.unet.ctx_dim:
            raise RuntimeError("text encoder widths do not add up to the UNet cross_attention_dim")

    @staticmethod
    def _text_encoders(eng):
        return list(eng.enc)

    @staticmethod
    def _text_bytes(eng):
        return sum(e.weight_bytes() for e in eng.enc)

    @staticmethod
    def _conditioning(eng, reqs, width, height, guidance, lane=0):
        prompts = [r.prompt for r in reqs]
        _, enc = eng._lane_encoders(lane)
        h1 = enc[0].forward(eng.tok[0](prompts), output="penultimate")
        h2, pooled = enc[1].forward(eng.tok[1](prompts), output="penultimate", pooled=True)
        pe = torch.cat([h1, h2], dim=-1)
        tids = torch.tensor([[float(height), float(width), 0.0, 0.0, float(height), float(width)]] * len(reqs))
        kw = dict(added=(pooled, tids))
        if guidance > 1.0 and not eng.pipe.unet.has_cond:
            kw["negative_embeds"] = torch.zeros_like(pe)
            kw["negative_added"] = (torch.zeros_like(pooled), tids)
        return pe, kw
