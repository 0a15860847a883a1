"""The LCM sampler on the MI355X: the arithmetic under ``self.pipe(...)`` (backends/cuda_worker.py:221-229)
as one hipGraph of hand-written HIP kernels.

Per request batch: prompt embeddings [B,77,768] + per-request seeds -> uint8 RGB [B,H,W,3] (+ final latents).
Order of operations follows backends/rknnlcm.py:450-647 (prompt embeds -> guidance embedding -> timesteps ->
latents from the request's generator -> [UNet -> LCMScheduler.step] x n -> /scaling_factor -> VAE -> u8).

RNG contract: each request owns a CPU ``torch.Generator`` seeded with its seed; draws are
latents[1,4,h,w] then one noise tensor per non-final step.  All draws happen on the host BEFORE the graph is
launched, so the captured graph is RNG-free and replays for any seed.

A hires request (``generate(..., hires=)``) keeps that one generator: it draws the plain request's tensors first --
latents[1,4,h,w], then steps - 1 step noises -- and then, at the target shape, the re-noise tensor [1,4,H2/8,W2/8] and
hr_steps - 1 step noises (``draw_noise_hires``).  Its bytes therefore depend only on (prompt, seed, size, steps, guidance, style,
target size, hr_steps, strength, mode) -- not on the batch, the lane or what ran before.

A variation (``generate(..., variation=)``; backends/variation.py) leaves that generator alone: G(seed) draws, exactly as above, the
target-shape tensor x [1,4,h,w] and then the step noises.  The variation adds generators of its own (``draw_variation``):
sub = randn(G'(subseed), [1,4,hs,ws]) and, only when a seed-resize is active, base = randn(G''(seed), [1,4,hs,ws]) -- a fresh
generator seeded with the request's seed; otherwise base is x itself and (hs, ws) = (h, w).  Both are multiplied by
init_noise_sigma like x.  lcm_noise_variation_f32 blends sub into base and pastes the result into x on the lane's stream, ahead of
the captured pass; step noises are never blended.  These draws, too, happen on the host before anything is launched.

A request with a sampler (``generate(..., sampler=)``, ``generate_img2img(..., sampler=)``; samplers.py) draws exactly the tensors
the same request draws without one.  Euler a reads the step noises, in draw order; Euler, DDIM and DPM++ 2M ignore them.  The
initial latents are multiplied by sb(sigma_0) on the device, inside the captured pass and therefore after a variation's blend.
"""
from __future__ import annotations

import os
import threading

import numpy as np
import torch

from . import ops
from .config import TEXT_SEQ_LEN, VAE_SCALE_FACTOR
from .lib import LcmHipError
from .model import ControlNetHip, UNetHip, VAEDecoderHip, VAEEncoderHip
from .scheduler import LCMSchedule
from . import samplers as _samplers


def guidance_scale_embedding(w: np.ndarray, dim: int) -> np.ndarray:
    """w = guidance_scale - 1 per request (backends/rknnlcm.py:572, :651-677)."""
    w = np.asarray(w, dtype=np.float32) * 1000
    half = dim // 2
    f = np.exp(np.arange(half, dtype=np.float32) * -(np.log(10000.0) / (half - 1)))
    e = w[:, None] * f[None, :]
    e = np.concatenate([np.sin(e), np.cos(e)], axis=1)
    if dim % 2 == 1:
        e = np.pad(e, [(0, 0), (0, 1)])
    return e.astype(np.float32)


def sinusoid_host(values: np.ndarray, dim: int) -> np.ndarray:
    """diffusers Timesteps(dim, flip_sin_to_cos=True, freq_shift=0) of a flat array: [cos | sin] per value (SDXL add_time_proj)."""
    half = dim // 2
    f = np.exp(-np.log(10000.0) * np.arange(half, dtype=np.float32) / half)
    e = np.asarray(values, dtype=np.float32).reshape(-1, 1) * f[None, :]
    return np.concatenate([np.cos(e), np.sin(e)], axis=1).astype(np.float32)


def check_size(width: int, height: int) -> None:
    """What diffusers' check_inputs raises for the reference ("`height` and `width` have to be divisible by 8 ...";
    backends/rknnlcm.py:380-381 has the same rule and text), as an LcmHipError; pinned by tests/golden/worker_contract.json."""
    if width % 8 or height % 8 or width <= 0 or height <= 0:
        raise LcmHipError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")


def _draw(seed: int, *groups):
    """A request's RNG stream: one CPU generator seeded with ``seed``; per (h, w, count) group, in order, ``count`` fp32
    [1,4,h,w] tensors -> one list per group."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return [[torch.randn((1, 4, h, w), generator=g, dtype=torch.float32) for _ in range(int(n))] for h, w, n in groups]


def draw_noise(seed: int, h: int, w: int, n_extra: int, sigma: float = 1.0):
    (lat,), extra = _draw(seed, (h, w, 1), (h, w, n_extra))
    return lat * sigma, extra


def draw_noise_hires(seed: int, h: int, w: int, steps: int, h2: int, w2: int, hr_steps: int, sigma: float = 1.0):
    """A hires request's RNG stream (module docstring) -> (latents, the steps - 1 step noises at [1,4,h,w], the re-noise tensor
    followed by the hr_steps - 1 step noises at [1,4,h2,w2])."""
    (lat,), lo, hi = _draw(seed, (h, w, 1), (h, w, int(steps) - 1), (h2, w2, hr_steps))
    return lat * sigma, lo, hi


def draw_noise_img2img(seed: int, h: int, w: int, steps: int, sigma: float = 1.0):
    """An image-to-image request's RNG stream, all from its one seeded generator and in this order: e0, the posterior sample's
    draw; e1, the re-noise draw at the first timestep of the strength-cut schedule; then the steps - 1 step noises
    -> (e0, [e1, e2, ...]) (``steps`` tensors in the list), each fp32 [1,4,h,w].  ``sigma`` is accepted for symmetry with
    ``draw_noise`` and unused: neither draw is an initial latent, so nothing is multiplied by init_noise_sigma."""
    (e0,), rest = _draw(seed, (h, w, 1), (h, w, steps))
    return e0, rest


def draw_variation_sources(seed: int, subseed: int, hs: int, ws: int, sigma: float = 1.0, resized: bool = False):
    """The tensors a variation adds to a request's draws (module docstring), each from a generator of its own ->
    (sub, base | None): sub = randn(G'(subseed), [1,4,hs,ws]) sigma; base = randn(G''(seed), [1,4,hs,ws]) sigma when a seed-resize
    is active (``resized``), else None: the request's own initial latents are the base.  subseed None (strength 0, a seed-resize
    alone): sub is None, nothing is drawn for it."""
    sub = base = None
    if subseed is not None:
        (sub,), = _draw(subseed, (hs, ws, 1))
        sub = sub * sigma
    if resized:
        (base,), = _draw(seed, (hs, ws, 1))
        base = base * sigma
    return sub, base


def draw_variation(seed: int, subseed: int, h: int, w: int, hs: int, ws: int, sigma: float = 1.0, n_extra: int = 0):
    """A request with a variation, all of its draws -> (x, step noises, sub, base | None): x and the ``n_extra`` step noises are
    ``draw_noise(seed, h, w, n_extra, sigma)`` bit for bit (the request's generator is not touched by the variation); sub and base
    are ``draw_variation_sources`` at the source shape (hs, ws), base only when that shape is not (h, w)."""
    x, extra = draw_noise(seed, h, w, n_extra, sigma)
    sub, base = draw_variation_sources(seed, subseed, hs, ws, sigma, resized=(int(hs), int(ws)) != (int(h), int(w)))
    return x, extra, sub, base


MAX_MASK_BLUR = 32.0


def mask_blur_weights(sigma: float):
    """The inpainting mask's integer Gaussian (A1111's mask_blur: kernel size 2 r + 1 with r = int(2.5 sigma + 0.5)) -> (r,
    uint32 [2 r + 1]): w_k = floor(65536 g_k / sum g) with g_k = exp(-k^2 / (2 sigma^2)) in float64, the remainder added to the
    centre tap so that the weights sum to exactly 65536.  sigma 0 -> (0, [65536]): no blur."""
    sigma = float(sigma)
    r = int(2.5 * sigma + 0.5)
    if r <= 0:
        return 0, np.array([65536], dtype=np.uint32)
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    w = np.floor(65536.0 * g / g.sum()).astype(np.int64)
    w[r] += 65536 - int(w.sum())
    return r, w.astype(np.uint32)


_DEFAULT_WS = {}


def _default_workspace(device):
    """The device-wide split-K workspace of launches outside any pipeline lane (eager launches of tests / tools on foreign
    streams): one process-lifetime tensor per device, never a lane's."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    t = _DEFAULT_WS.get(key)
    if t is None:
        t = _DEFAULT_WS[key] = torch.empty(int(os.environ.get("LCM_SPLITK_DEFAULT_WS_MB", "256")) << 18, dtype=torch.float32, device=device)
    return t


def _new_workspace(device):
    # sized for a batch of 8 at 768x768 (472 MB) / SDXL 1024x1024 (fp32 [splits][M][N] of the largest split layer); a launch
    # that needs more fails loudly (a silently smaller split factor would change the numbers)
    return torch.empty(int(os.environ.get("LCM_SPLITK_WS_MB", "1024")) << 18, dtype=torch.float32, device=device)


class _Lane:
    """One sampler instance of a pipeline: a stream, executors with scratch of their own (weights shared), its plans /
    captured graphs and its split-K workspace.  Lanes of one pipeline run concurrently: a single batch-1 pass is a
    chain of ~1700 latency-bound launches that leaves a third of the MI355X idle, so two requests in flight on two
    lanes finish in less than twice the time of one."""

    def __init__(self, pipe, index, unet, vae):
        self.index = index
        self.unet, self.vae = unet, vae
        self.stream = ops.acquire_stream(pipe.device)       # a handle of this lane's own (not torch's recycled pool)
        self.plans = {}
        # The split-K workspace belongs to THIS lane of THIS pipeline (the library looks it up by launch stream): two
        # pipelines on one GPU -- an SD1.5 and an SDXL engine, or unshared engines of several pool workers -- run on threads
        # with no common lock and must never share fp32 slabs.  It lives as long as the lane (i.e. as the captured graphs that
        # bake its pointer in) and is unregistered by LcmHipPipeline.close().
        self.splitk_ws = _new_workspace(pipe.device)
        ops.set_stream_workspace(self.stream, self.splitk_ws)
        self.controlnet = None        # this lane's executor of the pipeline's ControlNet (LcmHipPipeline.lane_controlnet)
        self._controlnet_of = None
        self.vae_enc = None           # this lane's executor of the VAE encoder (LcmHipPipeline.lane_vae_encoder)
        self.fit_src = self.fit_ws = None      # uploads of another size (backends/fit.py): the raw picture and the resampler's workspace
        self.pre_ws = None            # ControlNet preprocessor (generate(preprocess=)): the Canny workspace, sized on first use
        self.enc_plans = {}           # (B, H, W) -> _EncPlan: the encoder stage of image-to-image requests
        self.var_h = self.var_d = None         # variations (generate(variation=)): pinned / device staging of sub and base, sized on first use
        # SD upscale (backends/sdupscale.py): the decoded tiles of the request in flight, the combined picture and its pinned
        # read-back buffer; sized on first use, grown on demand
        self.grid_tiles = self.grid_out = self.h_grid = None


class _Plan:
    """Buffers + captured graph for one (B, h, w, steps, cfg) key.  refine = (strength, passes to run, starts from cached
    latents) makes it the plan of a refinement chain; None: the plain sampler (LcmHipPipeline._enqueue runs both).  The two stages of a hires request
    are plan kinds of their own: kind "latents" is the plain sampler without the VAE decode and the RGB epilogue (its result is
    P.lat), kind "from-state" a started-from-latents refinement plan whose first state the hand-over launch has already written
    to P.lat.  Kind "inpaint" is a from-state plan of its own (image-to-image plans and graphs are untouched by it): it owns the
    mask's device buffers, steps with lcm_scheduler_step_inpaint and overlays the picture after the decode."""

    FROM_STATE = ("from-state", "inpaint")

    def __init__(self, pipe, B, h, w, steps, do_cfg, lane=None, refine=None, control=None, kind=None, n_ctx=1, sampler=None):
        # Every zero-fill below must be ordered before the first use on the lane's (non-blocking) stream: allocate
        # under that stream, or a fill still queued on the null stream can land AFTER the request's uploads.
        self.lane = lane if lane is not None else pipe.lanes[0]
        self.refine = refine
        self.control = control        # conditioning scale of a ControlNet plan (baked into the captured GEMMs); None: no hint
        self.kind = kind              # None | "latents" | "from-state" (the stages of a hires request) | "inpaint"
        self.init_img = None          # inpaint: the encoder stage's picture buffer (uint8 [B,H,W,3]), set by generate_inpaint
        self.n_ctx = int(n_ctx)       # 77-token chunks of the prompt: the cross-attention context is 77 n_ctx rows per image
        # samplers.Tables of an Euler / Euler a / DDIM / DPM++ 2M plan (the pass is LcmHipPipeline._sampler_pass); None: LCM
        self.sampler = None
        if sampler is not None:
            name, schedule = sampler
            try:
                self.sampler = (_samplers.img2img_tables(pipe.sched, name, schedule, steps, refine[0]) if kind in self.FROM_STATE
                                else _samplers.tables(pipe.sched, name, schedule, steps))
            except ValueError as e:
                raise LcmHipError(str(e))
        with torch.cuda.stream(self.lane.stream):
            self._init(pipe, B, h, w, steps, do_cfg)
            if self.sampler is not None:          # the previous step's x0 (DPM++ 2M reads it; every step writes it)
                self.x0_prev = torch.zeros(B, 4, h, w, dtype=torch.float32, device=pipe.device)

    def _init(self, pipe, B, h, w, steps, do_cfg):
        dev = pipe.device
        self.B, self.h, self.w, self.steps, self.do_cfg = B, h, w, steps, do_cfg
        UB = 2 * B if do_cfg else B
        self.UB = UB
        self.ehs = torch.zeros(UB * TEXT_SEQ_LEN * self.n_ctx, pipe.unet.ctx_dim, dtype=torch.float16, device=dev)
        self.wemb = torch.zeros(UB, pipe.unet.cfg.get("time_cond_proj_dim") or 8, dtype=torch.float16, device=dev)
        self.add_in = (torch.zeros(UB, pipe.unet.added_dim, dtype=torch.float16, device=dev)
                       if pipe.unet.has_added else None)          # SDXL: [pooled text embeds | sinusoid(time ids)]
        self.lat0 = torch.zeros(B, 4, h, w, dtype=torch.float32, device=dev)         # request input
        self.lat = torch.zeros(UB, 4, h, w, dtype=torch.float32, device=dev)          # sampler state
        # noise tensors of the chain: the plain pass's steps - 1, then `steps` per refinement pass (its re-noise draw first)
        n_noise = max(steps - 1, 1)
        self.xk = None
        if self.refine is not None:
            _, run, cached = self.refine
            n_noise = max(run * steps + (0 if cached else steps - 1), 1)
            # xk[0]: the latents the chain starts from (uploaded from the cache, or the plain pass's x^0); xk[j]: j passes later
            self.xk = torch.zeros(run + 1, B, 4, h, w, dtype=torch.float32, device=dev)
        self.noise = torch.zeros(n_noise, B, 4, h, w, dtype=torch.float32, device=dev)
        self.eps = torch.zeros(UB, h, w, 4, dtype=torch.float32, device=dev)
        self.rgb = torch.zeros(B, h * VAE_SCALE_FACTOR, w * VAE_SCALE_FACTOR, 3, dtype=torch.uint8, device=dev)
        self.pool8 = torch.zeros(B, 4, 8, 8, dtype=torch.float16, device=dev)
        if self.control is not None:
            # the request's hint: a fixed device buffer of this plan (i.e. of this lane) that every replay uploads into, and
            # its embedding, written once per request by the hint stack inside the captured graph
            H8, W8 = h * VAE_SCALE_FACTOR, w * VAE_SCALE_FACTOR
            self.hint = torch.zeros(B, H8, W8, 3, dtype=torch.uint8, device=dev)
            self.h_hint = torch.zeros(B, H8, W8, 3, dtype=torch.uint8).pin_memory()
            self.hint_emb = torch.zeros(UB * h * w, pipe.unet.cfg["block_out_channels"][0], dtype=torch.float16, device=dev)
        if self.kind == "inpaint":
            H8, W8 = h * VAE_SCALE_FACTOR, w * VAE_SCALE_FACTOR
            self.mask, self.alpha, self.mask_tmp = (torch.zeros(B, H8, W8, dtype=torch.uint8, device=dev) for _ in range(3))
            self.latmask = torch.zeros(B, h, w, dtype=torch.uint8, device=dev)
            self.h_mask = torch.zeros(B, H8, W8, dtype=torch.uint8).pin_memory()
            self.h_alpha = torch.zeros(B, H8, W8, dtype=torch.uint8).pin_memory()
            self.h_latmask = torch.zeros(B, h, w, dtype=torch.uint8).pin_memory()
        self.img_f32 = None
        self.guidance = 1.0
        self.graph = None
        # pinned staging for H2D / D2H
        self.h_lat = torch.zeros(B, 4, h, w, dtype=torch.float32).pin_memory()
        self.h_noise = torch.zeros(n_noise, B, 4, h, w, dtype=torch.float32).pin_memory()
        self.h_rgb = torch.zeros(B, h * VAE_SCALE_FACTOR, w * VAE_SCALE_FACTOR, 3, dtype=torch.uint8).pin_memory()
        self.h_pool8 = torch.zeros(B, 4, 8, 8, dtype=torch.float16).pin_memory()
        self.h_latout = torch.zeros(B, 4, h, w, dtype=torch.float32).pin_memory()


class _EncPlan:
    """The encoder stage of image-to-image requests of one (lane, B, H, W): the picture's fixed device buffer, the posterior
    sample's noise, and the captured graph of VAEEncoderHip.encode (its outputs live in the lane executor's scratch)."""

    def __init__(self, pipe, lane, B, H, W):
        dev = pipe.device
        h, w = H // VAE_SCALE_FACTOR, W // VAE_SCALE_FACTOR
        self.B, self.H, self.W = B, H, W
        with torch.cuda.stream(lane.stream):
            self.img = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev)
            self.e0 = torch.zeros(B, 4, h, w, dtype=torch.float32, device=dev)
            self.moments = torch.zeros(B, 8, h, w, dtype=torch.float32, device=dev)
        self.h_img = torch.zeros(B, H, W, 3, dtype=torch.uint8).pin_memory()
        self.h_e0 = torch.zeros(B, 4, h, w, dtype=torch.float32).pin_memory()
        self.h_z = torch.zeros(B, 4, h, w, dtype=torch.float32).pin_memory()
        self.graph = None
        self.pre = None               # (pre_mean, pre_logvar): set by the first eager run, the same tensors ever after


class LcmHipPipeline:
    def __init__(self, unet_sd, vae_sd, unet_cfg=None, vae_cfg=None, device="cuda:0", schedule: LCMSchedule | None = None,
                 use_graph=True):
        if not torch.cuda.is_available():
            raise LcmHipError("LcmHipPipeline needs an MI355X (torch.cuda.is_available() is False); "
                              "there is no CPU fallback on the product path")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.unet = UNetHip(unet_sd, unet_cfg, self.device)
        self.vae = VAEDecoderHip(vae_sd, vae_cfg, self.device)
        self.sched = schedule or LCMSchedule()
        self.use_graph = use_graph
        self._tuned_keys = set()
        self._build_lock = threading.RLock()      # tuning / eager warm-up / capture of a plan: one lane at a time
        self.controlnet = None
        self.vae_encoder = None                   # VAEEncoderHip, built on the first image-to-image request
        self.vae_encoder_src = None               # (host state dict with encoder.* / quant_conv.*, VAE config) or None
        self._blur_weights = {}                   # mask_blur -> (radius, device uint32 weights) of inpaint requests
        self.lanes = [_Lane(self, 0, self.unet, self.vae)]
        self.stream = self.lanes[0].stream
        self._plans = self.lanes[0].plans
        # fp32 scratch for deterministic split-K of the deep-K / small-M layers (low-res UNet levels at batch 1): per lane
        # (above); launches on streams that are no lane's (tests, tools) use a device-wide default that no lane shares.
        self._splitk_ws = self.lanes[0].splitk_ws
        ops.set_workspace(_default_workspace(self.device))
        # A/B switches for kernel work.  LCM_ATTN_KSPLIT=0: unsplit streaming attention at every length (changes the bits of the
        # >= 1024-key levels)
        for env, setter in (("LCM_CONV_IMPL", ops.set_conv_impl), ("LCM_GN_FUSED_BYTES", ops.set_gn_fused_bytes),
                            ("LCM_PERSIST_N", ops.set_persist_n), ("LCM_HALO_PIPE", ops.set_halo_pipe_threshold),
                            ("LCM_ATTN_KSPLIT", ops.set_attention_ksplit), ("LCM_KERNEL_VARIANT", ops.set_kernel_variant)):
            if env in os.environ:
                setter(int(os.environ[env]))

    # ------------------------------------------------------------------------------------------
    def lane(self, index: int) -> _Lane:
        """Lane ``index`` (created on first use: executor views + stream + workspace; weights are shared)."""
        with self._build_lock:
            while len(self.lanes) <= index:
                self.lanes.append(_Lane(self, len(self.lanes), self.unet.view(), self.vae.view()))
        return self.lanes[index]

    def set_controlnet(self, sd, cfg=None):
        """Load a ControlNet (diffusers ControlNetModel state dict + config) beside the UNet; None releases it.  It must fit
        the UNet (weights.check_controlnet_matches raises otherwise).  Plans with a hint are dropped: they bake its pointers in."""
        with self._build_lock:
            for L in self.lanes:
                self._close_graphs(L, lambda P: P.control is not None)
                L.controlnet = L._controlnet_of = None
            self.controlnet = None if sd is None else ControlNetHip(sd, cfg, self.unet.cfg, self.device)
        return self.controlnet

    def lane_controlnet(self, L: _Lane):
        """The lane's executor of the ControlNet: weights shared, scratch of its own (like the UNet's views)."""
        if self.controlnet is None:
            raise LcmHipError("this request carries a ControlNet hint but no ControlNet is loaded (set_controlnet)")
        if L._controlnet_of is not self.controlnet:
            L.controlnet = self.controlnet if L.index == 0 else self.controlnet.view()
            L._controlnet_of = self.controlnet
        return L.controlnet

    def set_vae_encoder_source(self, sd, cfg=None):
        """Where the VAE encoder comes from: the ``encoder.*`` / ``quant_conv.*`` tensors of the checkpoint (host) and its VAE
        config.  Nothing is uploaded until an image-to-image request arrives."""
        self.vae_encoder_src = (sd, cfg) if sd else None

    def lane_vae_encoder(self, L: _Lane):
        """The lane's executor of the VAE encoder, built (and uploaded) on first use: weights shared, scratch per lane."""
        if self.vae_encoder is None:
            with self._build_lock:
                if self.vae_encoder is None:
                    if not self.vae_encoder_src:
                        raise LcmHipError("init_image: this checkpoint carries no VAE encoder (encoder.* / quant_conv.* tensors)")
                    sd, cfg = self.vae_encoder_src
                    sd = sd() if callable(sd) else sd
                    if not sd or "encoder.conv_in.weight" not in sd or "quant_conv.weight" not in sd:
                        raise LcmHipError("init_image: this checkpoint carries no VAE encoder (encoder.* / quant_conv.* tensors)")
                    from .weights import audit_vae_encoder
                    sd = audit_vae_encoder(sd, cfg if cfg is not None else self.vae.cfg)
                    with torch.cuda.stream(self.stream):
                        self.vae_encoder = VAEEncoderHip(sd, cfg if cfg is not None else self.vae.cfg, self.device)
                        self.stream.synchronize()
        if L.vae_enc is None:
            L.vae_enc = self.vae_encoder if L.index == 0 else self.vae_encoder.view()
        return L.vae_enc

    def _enc_plan(self, L: _Lane, B, H, W) -> _EncPlan:
        E = L.enc_plans.get((B, H, W))
        if E is None:
            with self._build_lock:
                E = L.enc_plans.get((B, H, W))
                if E is None:
                    E = L.enc_plans[(B, H, W)] = _EncPlan(self, L, B, H, W)
        return E

    def _encode_stage(self, L: _Lane, E: _EncPlan, eager: bool):
        """VAEEncoderHip.encode of E.img on the current (the lane's) stream -> (pre_mean, pre_logvar).  The stage is a captured
        graph of its own per (lane, B, H, W) -- ~120 launches that depend on nothing but the picture, replayed like the sampler's;
        the first use runs it eagerly once (allocates the executor's scratch), then captures.  eager: plain launches."""
        enc = self.lane_vae_encoder(L)
        if eager or E.graph is None:
            with self._build_lock:
                pm, pl, h, w = enc.encode(E.img, E.B, E.H, E.W)
                E.pre = (pm, pl)
                if not eager and E.graph is None:
                    L.stream.synchronize()
                    g = ops.Graph()
                    with g:
                        enc.encode(E.img, E.B, E.H, E.W)
                    E.graph = g
            return E.pre
        E.graph.launch()
        return E.pre

    @torch.inference_mode()
    def generate_img2img(self, prompt_embeds, seeds, images_u8, width, height, steps, strength, guidance_scale=1.0,
                         negative_embeds=None, want_float=False, noises=None, lane=0, sampler=None, tiles=None):
        """Image-to-image with the semantics of diffusers' LatentConsistencyModelImg2ImgPipeline: images_u8 uint8 [B,H,W,3] at the
        request's size -> AutoencoderKL encoder -> z = (mean + exp(0.5 clamp(logvar, -30, 20)) e0) scaling_factor -> re-noised to
        the first timestep of ``timesteps(steps, strength)`` with e1 -> ``steps`` LCM steps over that schedule -> decode.  The
        front stage of the request (``_request``) is the encoder stage (its own captured graph; eager with want_float or
        use_graph=False) and lcm_vae_posterior_renoise into the state of the "from-state" plan.  noises: optional
        per-request ``draw_noise_img2img`` results.  Returns the usual dict plus ``init_latents`` (host fp32 [B,4,h,w]: z) and
        ``unet_evals`` = steps (doubled under classifier-free guidance); with want_float also ``image`` and ``moments`` (host fp32
        [B,8,h,w]: the posterior's mean | logvar).
        sampler = (name, "normal" | "karras") (samplers.py): the tail of that sampler's ``steps``-step schedule the strength leaves
        (``samplers.img2img_tables``) in place of the LCM pass, from z re-noised to the tail's first noise level with e1 by the same
        hand-over launch; the LCM bound on steps x strength does not apply.  The draws are the same; ``unet_evals`` counts the
        tail's evaluations.
        tiles = (store, k0, n): the pass serves tiles k0 .. k0 + n - 1 of an SD-upscale request (``grid_store``): the decoded
        pictures of its first n slots are copied device-to-device into the store behind the read-backs, on the lane's stream, and
        are not read back: the result's ``rgb`` is None."""
        torch.cuda.set_device(self.device)
        pe = torch.as_tensor(prompt_embeds)
        B = pe.shape[0]
        steps, strength = int(steps), float(strength)
        check_size(width, height)
        if self.unet.has_added:
            raise LcmHipError("image-to-image is not served for SDXL-family UNets")
        if not 0.0 < strength <= 1.0:
            raise LcmHipError(f"image-to-image strength {strength} outside (0, 1]")
        img, img_fit = self._sources(images_u8, B, (height, width, 3), "init images")
        do_cfg = self._do_cfg(guidance_scale, negative_embeds)
        h, w = height // VAE_SCALE_FACTOR, width // VAE_SCALE_FACTOR
        if sampler is None:
            ts = self.sched.timesteps(steps, strength)   # diffusers' error for steps > original_steps x strength, before any plan
            nsa, nsb = self.sched.renoise_coefficients(ts[0])
        P = self._from_state_plan(B, width, height, steps, strength, guidance_scale, lane, n_ctx=self._n_ctx(pe), sampler=sampler)
        if sampler is not None:
            nsa, nsb = P.sampler.start
        L = P.lane
        self.lane_vae_encoder(L)                         # raises for a checkpoint without an encoder, before anything is queued
        E = self._enc_plan(L, B, height, width)
        for b, s in enumerate(seeds):
            e0, rest = noises[b] if noises is not None else draw_noise_img2img(s, h, w, steps)
            if len(rest) != steps:
                raise LcmHipError(f"request {b}: 1 + {len(rest)} noise tensors drawn ahead, the chain needs 1 + {steps}")
            E.h_e0[b].copy_(e0[0])
            for i, n in enumerate(rest):
                P.h_noise[i, b].copy_(n[0])
        self._stage(E.h_img, img)

        def upload():
            E.img.copy_(E.h_img, non_blocking=True)
            self._fit_pending(L, img_fit, E.img)
            E.e0.copy_(E.h_e0, non_blocking=True)

        def front(eager):                                # encoder -> hand-over into the strength-cut pass's state
            pre_m, pre_l = self._encode_stage(L, E, eager)
            enc = L.vae_enc
            ops.vae_posterior_renoise(pre_m, pre_l, enc.w["quant.w"], enc.w["quant.b"], E.e0, P.noise[0],
                                      self.vae.cfg["scaling_factor"], nsa, nsb, P.xk[0], P.lat, B, h, w,
                                      moments=E.moments if want_float else None, dup=do_cfg)

        def more():
            E.h_z.copy_(P.xk[0], non_blocking=True)
            if tiles is not None:
                store, k0, n = tiles
                store[k0:k0 + n].copy_(P.rgb[:n], non_blocking=True)

        if tiles is not None:
            store, k0, n = tiles
            if (store.dtype != torch.uint8 or tuple(store.shape[1:]) != (height, width, 3) or not 1 <= n <= B
                    or not 0 <= k0 <= store.shape[0] - n):
                raise LcmHipError(f"tiles {k0} .. {k0 + n - 1} of a pass of {B} do not fit a store of {tuple(store.shape)} {store.dtype}")
        out, _ = self._request([P], pe, negative_embeds, guidance_scale, upload, front, want_float=want_float, more=more,
                               read_rgb=tiles is None)
        out.update(init_latents=E.h_z.numpy().copy(),
                   unet_evals=(steps if sampler is None else len(P.sampler.ts)) * (2 if do_cfg else 1))
        if want_float:
            out["moments"] = E.moments.cpu().numpy()
        return out

    def _mask_weights(self, mask_blur):
        """(radius, device uint32 weights) of a mask blur: uploaded once per value and kept (the launches bake the pointer in)."""
        key = round(float(mask_blur), 6)
        got = self._blur_weights.get(key)
        if got is None:
            with self._build_lock:
                got = self._blur_weights.get(key)
                if got is None:
                    r, w = mask_blur_weights(key)
                    got = self._blur_weights[key] = (r, torch.from_numpy(w.astype(np.int64)).to(torch.int32).to(self.device)
                                                     if r > 0 else None)
        return got

    @torch.inference_mode()
    def generate_inpaint(self, prompt_embeds, seeds, images_u8, masks_u8, width, height, steps, strength, mask_blur=4.0,
                         guidance_scale=1.0, negative_embeds=None, want_float=False, noises=None, lane=0):
        """Inpainting: ``generate_img2img`` (the same encoder stage, posterior hand-over, strength-cut schedule and RNG stream,
        ``draw_noise_img2img``) with a mask.  masks_u8 uint8 [B,H,W] at the request's size, 255 = repaint.  On the device
        (lcm_inpaint_mask_prepare) the mask is blurred with A1111's Gaussian of sigma ``mask_blur`` in integer arithmetic -> alpha,
        and reduced 8 x 8 to the binary latent mask M (block mean >= 127.5).  After every scheduler step the latents outside M are
        put back on the init picture's own noised trajectory -- z re-noised with e1 to the next timestep, z itself after the last
        step (diffusers' StableDiffusionInpaintPipeline, 4-channel UNet) -- by lcm_scheduler_step_inpaint, which is the step
        launch of the pass.  After the decode the uploaded picture is laid over the result per pixel:
        out = (alpha gen + (255 - alpha) init + 127) / 255 (lcm_inpaint_composite_rgb8).  Returns generate_img2img's dict (``rgb``
        is the overlaid picture; with want_float ``image`` is the decode before the overlay) plus ``alpha`` (host uint8 [B,H,W])
        and ``latent_mask`` (host uint8 [B,h,w])."""
        torch.cuda.set_device(self.device)
        pe = torch.as_tensor(prompt_embeds)
        B = pe.shape[0]
        steps, strength, mask_blur = int(steps), float(strength), float(mask_blur)
        check_size(width, height)
        if self.unet.has_added:
            raise LcmHipError("inpainting is not served for SDXL-family UNets")
        if not 0.0 < strength <= 1.0:
            raise LcmHipError(f"inpainting strength {strength} outside (0, 1]")
        if not 0.0 <= mask_blur <= MAX_MASK_BLUR:
            raise LcmHipError(f"mask_blur {mask_blur} outside [0, {MAX_MASK_BLUR:g}]")
        img, img_fit = self._sources(images_u8, B, (height, width, 3), "init images")
        msk, msk_fit = self._sources(masks_u8, B, (height, width), "masks")
        do_cfg = self._do_cfg(guidance_scale, negative_embeds)
        ts = self.sched.timesteps(steps, strength)       # diffusers' error for steps > original_steps x strength, before any plan
        nsa, nsb = self.sched.renoise_coefficients(ts[0])
        h, w = height // VAE_SCALE_FACTOR, width // VAE_SCALE_FACTOR
        P = self._from_state_plan(B, width, height, steps, strength, guidance_scale, lane, kind="inpaint", n_ctx=self._n_ctx(pe))
        L = P.lane
        self.lane_vae_encoder(L)                         # raises for a checkpoint without an encoder, before anything is queued
        E = self._enc_plan(L, B, height, width)
        P.init_img = E.img                               # one buffer per (lane, B, H, W), as long-lived as the plan's graph
        radius, wts = self._mask_weights(mask_blur)
        for b, s in enumerate(seeds):
            e0, rest = noises[b] if noises is not None else draw_noise_img2img(s, h, w, steps)
            if len(rest) != steps:
                raise LcmHipError(f"request {b}: 1 + {len(rest)} noise tensors drawn ahead, the chain needs 1 + {steps}")
            E.h_e0[b].copy_(e0[0])
            for i, n in enumerate(rest):
                P.h_noise[i, b].copy_(n[0])
        self._stage(E.h_img, img)
        self._stage(P.h_mask, msk)

        def upload():
            E.img.copy_(E.h_img, non_blocking=True)
            self._fit_pending(L, img_fit, E.img)
            E.e0.copy_(E.h_e0, non_blocking=True)
            P.mask.copy_(P.h_mask, non_blocking=True)
            self._fit_pending(L, msk_fit, P.mask)

        def front(eager):                                # encoder -> mask -> hand-over into the masked pass's state
            pre_m, pre_l = self._encode_stage(L, E, eager)
            enc = L.vae_enc
            ops.inpaint_mask_prepare(P.mask, wts, radius, P.alpha, P.mask_tmp, P.latmask, B, height, width)
            ops.vae_posterior_renoise(pre_m, pre_l, enc.w["quant.w"], enc.w["quant.b"], E.e0, P.noise[0],
                                      self.vae.cfg["scaling_factor"], nsa, nsb, P.xk[0], P.lat, B, h, w,
                                      moments=E.moments if want_float else None, dup=do_cfg)

        def more():
            E.h_z.copy_(P.xk[0], non_blocking=True)
            P.h_alpha.copy_(P.alpha, non_blocking=True)
            P.h_latmask.copy_(P.latmask, non_blocking=True)

        out, _ = self._request([P], pe, negative_embeds, guidance_scale, upload, front, want_float=want_float, more=more)
        out.update(init_latents=E.h_z.numpy().copy(), alpha=P.h_alpha.numpy().copy(), latent_mask=P.h_latmask.numpy().copy(),
                   unet_evals=steps * (2 if do_cfg else 1))
        if want_float:
            out["moments"] = E.moments.cpu().numpy()
        return out

    def _enqueue(self, P: _Plan, guidance: float, want_float=False, taps=None):
        """Enqueue the whole sampler on the current stream (this is what gets captured): a chain of passes, each the LCM steps
        over one schedule.  A plain plan is the one pass over timesteps(steps).  A refinement plan P.refine = (d, run, cached) is
        that pass (unless the chain starts from cached latents in P.xk[0], re-noised by lcm_latents_renoise) followed by `run`
        passes over the strength-cut schedule.  A pass that another one follows ends in the hand-over step (x^k to P.xk, the
        re-noised state of the next pass to P.lat, one launch); the last pass ends in the plain `last` step and only its x goes
        through the VAE.  A plan with a sampler (P.sampler) is one pass of ``_sampler_pass`` instead, decoded the same way."""
        if P.sampler is not None:
            return self._decode(P, self._sampler_pass(P, guidance, taps), want_float, taps)
        B, UB, h, w = P.B, P.UB, P.h, P.w
        unet, vae = P.lane.unet, P.lane.vae
        pred = self.sched.prediction_type
        d, run, cached = P.refine if P.refine is not None else (1.0, 0, False)
        passes = [] if cached else [self.sched.timesteps(P.steps)]
        nsa = nsb = None
        if run:
            ts_cut = self.sched.timesteps(P.steps, d)
            nsa, nsb = self.sched.renoise_coefficients(ts_cut[0])
            passes += [ts_cut] * run
        ni = 0                                        # next tensor of P.noise, in draw order
        if taps is not None and not cached:
            taps["latents0"] = P.lat0.cpu()           # the initial latents as the pass reads them (after a variation's blend)
        if cached:
            if P.kind not in P.FROM_STATE:            # hires stage 2: lcm_latents_upscale_renoise wrote P.lat (and P.xk[0])
                ops.latents_renoise(P.xk[0], P.noise[0], nsa, nsb, P.lat, B, h, w, dup=P.do_cfg)
            ni = 1
        elif P.do_cfg:
            P.lat[:B].copy_(P.lat0)
            P.lat[B:].copy_(P.lat0)
        else:
            P.lat.copy_(P.lat0)
        kv = unet.encode_context(P.ehs, UB)
        aug = unet.encode_added(P.add_in, UB) if unet.has_added else None
        wemb = P.wemb if unet.has_cond else None
        # under classifier-free guidance rows [0,B) = negative prompt, [B,2B) = prompt: the step updates the prompt half
        state = P.lat[B:] if P.do_cfg else P.lat
        eps = P.eps[B:] if P.do_cfg else P.eps
        kw = dict(eps_uncond=P.eps[:B], guidance=guidance) if P.do_cfg else {}

        def hoist(net, ts, wemb, aug):
            # the time-embedding MLP + all time_emb_proj of EVERY step of a pass ahead of its steps (they depend on the schedule
            # and the request's guidance only): 5 launches per pass instead of 4 per step; None: per step, inside forward
            return net.time_embed_all([int(t) for t in ts], wemb, UB, aug) if len(ts) <= net.MAX_HOISTED_STEPS else None

        ta_all, ta_c, ta_ts = hoist(unet, passes[0], wemb, aug), None, passes[0]
        cn = None
        if P.control is not None:
            cn, kv_c = self._control_setup(P, taps)
            ta_c = hoist(cn, passes[0], None, None)
        for j, ts in enumerate(passes):
            if list(ts) != list(ta_ts):               # once per distinct schedule, reused across consecutive equal passes
                ta_all, ta_ts = hoist(unet, ts, wemb, aug), ts
                if cn is not None:
                    ta_c = hoist(cn, ts, None, None)
            for i, t in enumerate(ts):
                rows, tap1 = slice(i * UB, (i + 1) * UB), taps if (i == 0 and j == 0) else None
                control = None
                if cn is not None:
                    feats, mid_f = cn.forward(P.lat, int(t), kv_c, UB, h, w, P.hint_emb, taps=tap1,
                                              ta=ta_c[rows] if ta_c is not None else None)
                    control = (cn, feats, mid_f, P.control)
                unet.forward(P.lat, int(t), kv, wemb, UB, h, w, P.eps, taps=tap1, aug=aug,
                             ta=ta_all[rows] if ta_all is not None else None, control=control)
                coef, last = self.sched.step_coefficients(ts, i)
                if P.kind == "inpaint":               # the step and the select in one launch; both halves under guidance
                    # kept cells follow the init picture: z (P.xk[0]) re-noised with e1 (P.noise[0]; the step noises follow it) to
                    # the next timestep, z itself at the end
                    ksa, ksb = (1.0, 0.0) if last else self.sched.renoise_coefficients(ts[i + 1])
                    ops.scheduler_step_inpaint(eps, state, P.noise[min(ni, P.noise.shape[0] - 1)], P.xk[0], P.noise[0], P.latmask,
                                               coef, last, ksa, ksb, B, h, w, pred=pred, dup=P.do_cfg, **kw)
                    ni += 0 if last else 1
                elif last and j < len(passes) - 1:
                    ops.scheduler_step_handover(eps, state, P.noise[ni], P.xk[j + 1 if cached else j], coef, nsa, nsb, B, h, w,
                                                pred=pred, dup=P.do_cfg, **kw)
                    ni += 1
                else:                                 # the final `last` step reads no noise: any tensor of P.noise serves
                    ops.scheduler_step(eps, state, P.noise[min(ni, P.noise.shape[0] - 1)], coef, last, B, h, w, pred=pred, **kw)
                    if not last:
                        ni += 1
                        if P.do_cfg:
                            P.lat[:B].copy_(state)
        if P.xk is not None:
            P.xk[run].copy_(state)
        if P.kind == "latents":                       # hires stage 1: nobody sees this picture, so nothing decodes it
            return state
        return self._decode(P, state, want_float, taps)

    def _control_setup(self, P: _Plan, taps=None):
        """The part of a ControlNet plan's pass that is done once per request -> (the lane's ControlNet executor, its
        cross-attention K/V): the hint embedding (it depends on the hint alone), repeated for the unconditional half under
        classifier-free guidance (diffusers' guess_mode=False), and the ControlNet's own K/V of the prompt."""
        B, h, w = P.B, P.h, P.w
        cn = self.lane_controlnet(P.lane)
        n1 = B * h * w
        cn.embed_hint(P.hint, B, h * VAE_SCALE_FACTOR, w * VAE_SCALE_FACTOR, P.hint_emb[:n1])
        if P.do_cfg:
            P.hint_emb[n1:].copy_(P.hint_emb[:n1])
        if taps is not None:
            taps["cn.hint_emb"] = P.hint_emb[:n1].reshape(B, h, w, -1).permute(0, 3, 1, 2).float().cpu()
        return cn, cn.encode_context(P.ehs, P.UB)

    def _decode(self, P: _Plan, state, want_float=False, taps=None):
        """The end of every pass that shows a picture: the pooled latents, the VAE decode and the RGB epilogue."""
        B, h, w, vae = P.B, P.h, P.w, P.lane.vae
        ops.latents_pool8(state, P.pool8, B, h, w)
        if want_float and P.img_f32 is None:
            P.img_f32 = torch.zeros(B, h * 8, w * 8, 3, dtype=torch.float32, device=self.device)
        vae.decode(state, B, h, w, P.rgb, img_f32=P.img_f32 if want_float else None, taps=taps)
        if P.kind == "inpaint":                       # the uploaded picture shows through where alpha < 255 (P.img_f32 stays the decode)
            ops.inpaint_composite_rgb8(P.rgb, P.init_img, P.alpha, B, h * VAE_SCALE_FACTOR, w * VAE_SCALE_FACTOR)
        return state

    def _sampler_pass(self, P: _Plan, guidance: float, taps=None):
        """The pass of a plan with a sampler (P.sampler: samplers.Tables; include/lcm_hip.h, samplers): Euler, Euler a, DDIM or
        DPM++ 2M over the plan's own noise levels -- a plain or ControlNet plan from the initial latents, a from-state plan
        (image-to-image) from the state the posterior hand-over wrote.  The initial noise is scaled by sb(sigma_0) HERE, on the
        device and inside the captured graph, i.e. after a variation's blend into P.lat0 (lcm_latents_renoise with weight 0 on
        its second operand: one launch that also fills both classifier-free halves); DDIM starts from the noise itself.  The
        UNet -- and the ControlNet -- are evaluated at the step's fractional timestep: nothing truncates it.  Every step is one
        lcm_sampler_step launch; under classifier-free guidance it writes both halves of the state.  Euler a reads the
        request's step noises in draw order; the deterministic samplers read none.  -> the state (the prompt half)."""
        T = P.sampler
        B, UB, h, w = P.B, P.UB, P.h, P.w
        unet = P.lane.unet
        pred = self.sched.prediction_type
        from_state = P.kind in P.FROM_STATE
        ni = 1 if from_state else 0                   # P.noise[0] of a from-state plan is e1, the hand-over's draw
        if not from_state:                            # (a from-state plan: lcm_vae_posterior_renoise wrote P.lat and P.xk[0])
            if taps is not None:
                taps["latents0"] = P.lat0.cpu()       # the initial latents as the pass reads them (after a variation's blend)
            if T.init_scale is not None:
                ops.latents_renoise(P.lat0, P.lat0, T.init_scale, 0.0, P.lat, B, h, w, dup=P.do_cfg)
            elif P.do_cfg:
                P.lat[:B].copy_(P.lat0)
                P.lat[B:].copy_(P.lat0)
            else:
                P.lat.copy_(P.lat0)
        kv = unet.encode_context(P.ehs, UB)
        wemb = P.wemb if unet.has_cond else None
        state = P.lat[B:] if P.do_cfg else P.lat
        eps = P.eps[B:] if P.do_cfg else P.eps
        kw = dict(eps_uncond=P.eps[:B], guidance=guidance) if P.do_cfg else {}
        ts = [float(t) for t in T.ts]
        ta_all = unet.time_embed_all(ts, wemb, UB, None)          # len(ts) <= samplers.MAX_STEPS <= MAX_HOISTED_STEPS
        cn = ta_c = None
        if P.control is not None:
            cn, kv_c = self._control_setup(P, taps)
            ta_c = cn.time_embed_all(ts, None, UB, None)
        for i, t in enumerate(ts):
            rows, tap1 = slice(i * UB, (i + 1) * UB), taps if i == 0 else None
            control = None
            if cn is not None:
                feats, mid_f = cn.forward(P.lat, t, kv_c, UB, h, w, P.hint_emb, taps=tap1, ta=ta_c[rows])
                control = (cn, feats, mid_f, P.control)
            unet.forward(P.lat, t, kv, wemb, UB, h, w, P.eps, taps=tap1, ta=ta_all[rows], control=control)
            c_sa, c_sb, cx, c0, c1, c_n = T.coefs[i]
            ops.sampler_step(eps, state, P.x0_prev, P.noise[ni + i] if c_n != 0.0 else None, c_sa, c_sb, cx, c0, c1, c_n, B, h, w,
                             pred=pred, dup=P.do_cfg, **kw)
        if P.xk is not None:
            P.xk[1].copy_(state)
        return state

    def plan(self, B, h, w, steps, do_cfg=False, guidance=None, lane=0, refine=None, control=None, kind=None, n_ctx=1,
             sampler=None) -> _Plan:
        # classifier-free guidance bakes the guidance value into the captured step kernels: one plan per value
        key = (B, h, w, steps, do_cfg, round(float(guidance), 4) if do_cfg and guidance is not None else None)
        if refine is not None:                       # (d, passes to run, starts from cached latents): a chain of its own
            key = key + (round(float(refine[0]), 6), int(refine[1]), bool(refine[2]))
        if control is not None:                      # a ControlNet plan: "control" + the conditioning scale its GEMMs bake in
            key = key + ("control", round(float(control), 6))
        if kind is not None:                         # a stage of a hires request: "latents" (no decode) / "from-state"; "inpaint"
            key = key + (kind,)
        if int(n_ctx) != 1:                          # a long prompt: 77 n_ctx context rows (other buffers, other launches)
            key = key + ("ctx", int(n_ctx))
        if sampler is not None:                      # Euler / Euler a / DDIM / DPM++ 2M: (canonical name, "normal" | "karras")
            key = key + ("sampler", str(sampler[0]), str(sampler[1]))
        L = self.lane(lane)
        P = L.plans.get(key)
        if P is None:
            with self._build_lock:
                P = L.plans.get(key)
                if P is None:
                    P = _Plan(self, B, h, w, steps, do_cfg, L, refine=refine,
                              control=None if control is None else round(float(control), 6), kind=kind, n_ctx=n_ctx,
                              sampler=None if sampler is None else (str(sampler[0]), str(sampler[1])))
                    L.plans[key] = P
        return P

    def tune(self, P: _Plan, verbose=False):
        """Autotune the launch plan of every contraction shape this plan touches (once per shape per process)."""
        if os.environ.get("LCM_AUTOTUNE", "1") == "0" or getattr(P, "tuned", False):
            return
        from . import autotune
        stream = P.lane.stream
        with self._build_lock, torch.cuda.stream(stream):
            self._enqueue(P, 1.0)                    # allocate scratch, warm caches
            with ops.recording() as recs:            # thread-local: another lane's eager launches never land in here
                self._enqueue(P, 1.0)
            stream.synchronize()
            todo = [r for r in recs if r[0] is not None and r[0] not in self._tuned_keys]
            # in situ every layer's weights come from HBM and its input was written by the previous kernel, never by a
            # previous run of the same layer: time the candidates with cold caches (autotune._time_cold); measured
            # +2.5 % at batch 1 and +1.7 % at batch 8 over warm back-to-back timing.  LCM_AUTOTUNE_COLD=0: warm timing
            cold = os.environ.get("LCM_AUTOTUNE_COLD", "1") != "0"
            # LCM_TUNE_SPLITS=1: offline table generation only (tools/make_plans.py) -- a serving process never times splits
            res = autotune.autotune(todo, P.lane.splitk_ws.numel() * 4, verbose=verbose, cold=cold,
                                    tune_splits=os.environ.get("LCM_TUNE_SPLITS", "0") == "1")
            self._tuned_keys.update(res.keys())
            stream.synchronize()
        P.tuned = True

    @staticmethod
    def _close_graphs(L: _Lane, only=None):
        """Close and forget the captured graphs of a lane with their plans: sampler plans and encoder stages, or -- with
        only(P) -- just the sampler plans it picks."""
        for plans in (L.plans,) if only is not None else (L.plans, L.enc_plans):
            for key in [k for k, P in plans.items() if only is None or only(P)]:
                g = plans.pop(key).graph
                if g is not None:
                    g.close()

    def drop_plans(self):
        for L in self.lanes:
            self._close_graphs(L)

    def close(self):
        """Drop the captured graphs and take this pipeline's workspaces out of the library's per-stream table (the library
        keeps raw pointers).  Idempotent; also run when the pipeline is collected."""
        lanes, self.lanes = getattr(self, "lanes", []), []
        self.controlnet = None
        for L in lanes:
            self._close_graphs(L)
            try:
                torch.cuda.synchronize(self.device)
                ops.set_stream_workspace(L.stream, L.splitk_ws, forget=True)      # only if the entry is still this lane's
                ops.release_stream(L.stream)
                L.stream = None
            except Exception:
                pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def _upload_text(self, P: _Plan, pe, negative_embeds, guidance_scale):
        """Prompt embeddings (negative ones in front under classifier-free guidance) and the guidance embedding into the plan's
        buffers, on the current stream."""
        B, rows = P.B, P.B * TEXT_SEQ_LEN * P.n_ctx
        pe16 = pe.to(torch.float16).reshape(rows, -1)
        if P.do_cfg:
            ne16 = torch.as_tensor(negative_embeds).to(torch.float16).reshape(rows, -1)
            P.ehs[:rows].copy_(ne16, non_blocking=True)
            P.ehs[rows:].copy_(pe16, non_blocking=True)
        else:
            P.ehs.copy_(pe16, non_blocking=True)
        if self.unet.has_cond:
            gs = np.full((B,), float(guidance_scale) - 1.0, dtype=np.float32)
            P.wemb.copy_(torch.from_numpy(guidance_scale_embedding(gs, P.wemb.shape[1])).to(torch.float16),
                         non_blocking=True)

    def _upload_added(self, P: _Plan, added, negative_added):
        """SDXL: [pooled text embeds | sinusoid(time ids)] rows into the plan's buffer (the negative ones in front under
        classifier-free guidance; zero pooled embeds when none are given), on the current stream."""
        B, dim = P.B, self.unet.cfg["addition_time_embed_dim"]

        def _add_rows(a):
            pooled, tids = a
            pooled = torch.as_tensor(pooled).to(torch.float32).reshape(B, -1).cpu()
            sin = sinusoid_host(np.asarray(tids, dtype=np.float32).reshape(-1), dim)
            return torch.cat([pooled, torch.from_numpy(sin).reshape(B, -1)], dim=1).to(torch.float16)
        rows = _add_rows(added)
        if P.do_cfg:
            neg_rows = _add_rows(negative_added if negative_added is not None else (torch.zeros(B, rows.shape[1] - 6 * dim), added[1]))
            P.add_in[:B].copy_(neg_rows, non_blocking=True)
            P.add_in[B:].copy_(rows, non_blocking=True)
        else:
            P.add_in.copy_(rows, non_blocking=True)

    def _ensure_graph(self, P: _Plan, guidance_scale):
        """Tune, warm up (allocates every scratch buffer) and capture the plan's graph on its lane's stream, once."""
        if P.graph is None:
            with self._build_lock:
                if P.graph is None:
                    self.tune(P)
                    self._enqueue(P, guidance_scale)
                    P.lane.stream.synchronize()
                    g = ops.Graph()
                    with g:
                        self._enqueue(P, guidance_scale)
                    P.graph = g

    def _do_cfg(self, guidance_scale, negative_embeds=False) -> bool:
        """Does guidance_scale mean classifier-free guidance here (guidance above 1 on a UNet without a guidance embedding)?  A
        request passes its negative_embeds: None is then an error."""
        do_cfg = (guidance_scale > 1.0) and not self.unet.has_cond
        if do_cfg and negative_embeds is None:
            raise LcmHipError("classifier-free guidance needs negative_embeds")
        return do_cfg

    @staticmethod
    def _n_ctx(pe) -> int:
        """Chunks of a request's prompt embeddings [B, 77 n, ctx]."""
        rows = pe.shape[1] if pe.dim() == 3 else 0
        if rows < TEXT_SEQ_LEN or rows % TEXT_SEQ_LEN:
            raise LcmHipError(f"prompt embeddings of shape {tuple(pe.shape)}: expected [B, {TEXT_SEQ_LEN} n, ctx]")
        return rows // TEXT_SEQ_LEN

    def _from_state_plan(self, B, width, height, steps, strength, guidance_scale, lane, kind="from-state", n_ctx=1,
                         sampler=None) -> _Plan:
        """The plan of one strength-cut pass that starts from a state the hand-over launch of a front stage wrote (hires
        stage 2, image-to-image; kind "inpaint": the masked pass of an inpaint request)."""
        return self.plan(B, height // VAE_SCALE_FACTOR, width // VAE_SCALE_FACTOR, int(steps), self._do_cfg(guidance_scale),
                         guidance_scale, lane=lane, refine=(float(strength), 1, True), kind=kind, n_ctx=n_ctx, sampler=sampler)

    def _recorded_need(self, holder, L: _Lane, run) -> int:
        """_need_of one eager run() recorded on the lane's stream; remembered on ``holder`` (a plan)."""
        need = getattr(holder, "_splitk_need", None)
        if need is None:
            with self._build_lock, torch.cuda.stream(L.stream):
                with ops.recording() as recs:
                    run()
                L.stream.synchronize()
            need = holder._splitk_need = self._need_of(recs)
        return need

    def splitk_need(self, P: _Plan) -> int:
        """An upper bound of the split-K workspace bytes a pass of P's size needs PER IMAGE ROW of the UNet batch, from the plan's
        own launches: the K partition of a layer is a property of its per-image shape (include/lcm_hip.h, Determinism), so a
        batch of n needs at most n times this (a batched launch that fills the chip keeps the parts in registers and needs
        less).  P must be a batch-1 plan: one eager pass of it is recorded -- a pass that does not fit at batch 1 raises the
        library's error."""
        if P.B != 1:
            raise LcmHipError("splitk_need: a batch-1 plan, please")
        return self._recorded_need(P, P.lane, lambda: self._enqueue(P, 1.0))

    @staticmethod
    def _need_of(recs) -> int:
        """The largest fp32 slab set (bytes per image) among recorded launches: parts x rows per image x N x 4 of every
        splittable contraction whose canonical K partition has parts."""
        from . import autotune
        need = 0
        for key, meta, _ in recs:
            if key is None or not meta.get("splittable"):
                continue
            m_img = meta.get("m_img", key[1])
            sp = autotune._canonical_splits(key, meta, m_img)
            if sp > 1:
                need = max(need, 4 * sp * m_img * key[2])
        return need

    def encoder_splitk_need(self, width, height, lane=0) -> int:
        """splitk_need of the VAE encoder stage at width x height, per picture: one eager batch-1 encode is recorded.  The
        encoder's Downsample2D runs its canonical partition as split launch + reduce at every batch, so a batch of n needs n
        times this."""
        L = self.lane(lane)
        E = self._enc_plan(L, 1, height, width)
        enc = self.lane_vae_encoder(L)
        return self._recorded_need(E, L, lambda: enc.encode(E.img, 1, height, width))

    def _batch_cap(self, width, height, steps, strength, guidance_scale, lane, sizes, other_need=0, n_ctx=1, sampler=None) -> int:
        """The largest pass size of ``sizes`` at which the from-state pass at width x height -- and a stage of ``other_need``
        bytes per request before it on the same stream -- fits the lane's split-K workspace (at least the smallest: a batch-1
        pass that does not fit raises the library's loud error when it runs)."""
        P = self._from_state_plan(1, width, height, steps, strength, guidance_scale, lane, n_ctx=n_ctx, sampler=sampler)
        per_request = max(self.splitk_need(P) * (2 if P.do_cfg else 1), other_need)   # classifier-free guidance: two UNet rows
        fit = [n for n in sorted(sizes) if n * per_request <= P.lane.splitk_ws.numel() * 4]
        return fit[-1] if fit else min(sizes)

    def img2img_batch_cap(self, width, height, steps, strength, guidance_scale=1.0, lane=0, sizes=(1, 2, 4, 8), n_ctx=1,
                          sampler=None) -> int:
        """The largest pass size of ``sizes`` at which BOTH stages of an image-to-image request at width x height fit the lane's
        split-K workspace: the strength-cut pass (hires_batch_cap's count, doubled rows under classifier-free guidance) and the
        encoder stage.  The stages run one after the other on one stream, so the need is the larger of the two."""
        return self._batch_cap(width, height, steps, strength, guidance_scale, lane, sizes,
                               self.encoder_splitk_need(width, height, lane), n_ctx=n_ctx, sampler=sampler)

    def inpaint_batch_cap(self, width, height, steps, strength, guidance_scale=1.0, lane=0, sizes=(1, 2, 4, 8), n_ctx=1) -> int:
        """img2img_batch_cap for an inpaint request: its masked pass runs the same contractions as the image-to-image pass (the
        plan it asks is the image-to-image one) and the same encoder stage; the mask launches need no split-K workspace."""
        return self.img2img_batch_cap(width, height, steps, strength, guidance_scale, lane, sizes, n_ctx=n_ctx)

    def hires_batch_cap(self, width, height, hr_steps, strength, guidance_scale=1.0, lane=0, sizes=(1, 2, 4, 8), n_ctx=1) -> int:
        """The largest pass size of ``sizes`` whose second stage at width x height fits the lane's split-K workspace (at least
        the smallest: a batch-1 pass that does not fit raises the library's loud error when it runs)."""
        return self._batch_cap(width, height, hr_steps, strength, guidance_scale, lane, sizes, n_ctx=n_ctx)

    def _run_plan(self, P: _Plan, guidance_scale, eager, want_float=False, taps=None):
        """Run the plan now, on the current stream: plain launches under the build lock (they allocate scratch), or its graph."""
        if eager:
            with self._build_lock:
                self._enqueue(P, guidance_scale, want_float=want_float, taps=taps)
        else:
            P.graph.launch()

    def _request(self, plans, pe, negative_embeds, guidance_scale, upload=None, front=None, want_float=False, taps=None, more=None,
                 vary=None, read_rgb=True):
        """The one sequence of every request kind, on the lane's stream.  plans: every plan of the request, the last one gives
        the picture; their pinned staging (h_lat, h_noise) is filled.  upload(): the kind's own uploads (hint, picture, start
        latents, SDXL rows); vary(): a variation's upload and its one launch into the first plan's lat0 (``_stage_variation``; None
        for every request without one); front(eager): the stage ahead of the last plan and its hand-over launch; more():
        device-side copies to queue after the read-backs -> (base result dict, what more() returned).  read_rgb=False: the decoded
        pictures stay on the device (an SD-upscale pass: more() keeps them in the tile store) and the dict's "rgb" is None.  The rules:
          * noise is drawn on the host, by the caller, before anything is launched: the graphs are RNG-free;
          * the graphs of EVERY plan of the request are ensured before its uploads: a warm-up pass overwrites plan state;
          * eager launches (use_graph=False, want_float, taps) hold _build_lock: they allocate scratch;
          * everything runs on the lane's stream and nothing is copied to the host between the stages;
          * exactly one synchronize per call, after the read-backs."""
        P = plans[-1]
        eager = (not self.use_graph) or want_float or taps is not None
        stream = P.lane.stream
        with torch.cuda.stream(stream):
            if not eager:
                for Q in plans:
                    self._ensure_graph(Q, guidance_scale)
            for Q in plans:
                if Q.kind not in Q.FROM_STATE:           # a from-state plan's first state comes from the hand-over launch
                    Q.lat0.copy_(Q.h_lat, non_blocking=True)
                Q.noise.copy_(Q.h_noise, non_blocking=True)
                self._upload_text(Q, pe, negative_embeds, guidance_scale)
            if upload is not None:
                upload()
            if vary is not None:
                vary()
            if front is not None:
                front(eager)
            self._run_plan(P, guidance_scale, eager, want_float, taps)
            if read_rgb:
                P.h_rgb.copy_(P.rgb, non_blocking=True)
            P.h_pool8.copy_(P.pool8, non_blocking=True)
            P.h_latout.copy_(P.lat[P.B:] if P.do_cfg else P.lat, non_blocking=True)
            extra = more() if more is not None else None
            stream.synchronize()
        out = dict(rgb=P.h_rgb.numpy().copy() if read_rgb else None, latents=P.h_latout.numpy().copy(), pool8=P.h_pool8.numpy().copy())
        if want_float:
            out["image"] = P.img_f32.cpu().numpy()       # NHWC float, pre-clamp
        return out, extra

    @torch.inference_mode()
    def generate_hires(self, prompt_embeds, seeds, width, height, steps, hires, guidance_scale=1.0, negative_embeds=None,
                       want_float=False, noises=None, lane=0, variation=None):
        """Hires fix: sample at (width, height) for ``steps`` steps, upscale the denoised latents to (W2, H2) with latent upscaler
        ``mode`` (lib.UPSCALE_MODES), re-noise them to the first timestep of ``timesteps(hr_steps, strength)``, run ``hr_steps``
        steps there and decode once.  hires = (W2, H2, hr_steps, strength, mode).  The front stage of the request (``_request``)
        is the "latents" plan at the base size (no VAE decode) and lcm_latents_upscale_renoise into the state of the
        "from-state" refinement plan at the target size.  noises: optional per-request
        ``draw_noise_hires`` results.  variation: as ``generate``'s, blended into the initial latents of the low-resolution stage.  Returns the usual dict at the target size plus ``lowres_latents`` (host fp32 [B,4,h,w],
        the plain request's final latents bit for bit) and ``unet_evals`` = steps + hr_steps (doubled under classifier-free
        guidance); with want_float (eager launches) also ``image`` and ``upscaled_latents`` (host fp32 [B,4,H2/8,W2/8])."""
        torch.cuda.set_device(self.device)
        pe = torch.as_tensor(prompt_embeds)
        B = pe.shape[0]
        W2, H2, hr_steps, strength, mode = hires
        W2, H2, steps, hr_steps, strength, mode = int(W2), int(H2), int(steps), int(hr_steps), float(strength), int(mode)
        check_size(width, height)
        check_size(W2, H2)
        if self.unet.has_added:
            raise LcmHipError("hires fix is not served for SDXL-family UNets")
        if mode not in (0, 1, 2):
            raise LcmHipError(f"unknown latent upscaler mode {mode}: expected 0 (bilinear), 1 (bicubic) or 2 (nearest-exact)")
        if not (width <= W2 <= 4 * width and height <= H2 <= 4 * height):
            raise LcmHipError(f"hires target {W2}x{H2} outside [1, 4] x the base size {width}x{height}")
        do_cfg = self._do_cfg(guidance_scale, negative_embeds)
        self.sched.timesteps(steps)
        ts2 = self.sched.timesteps(hr_steps, strength)   # diffusers' error for hr_steps > original_steps x strength, before any plan
        nsa, nsb = self.sched.renoise_coefficients(ts2[0])
        h, w, h2, w2 = height // VAE_SCALE_FACTOR, width // VAE_SCALE_FACTOR, H2 // VAE_SCALE_FACTOR, W2 // VAE_SCALE_FACTOR
        n_ctx = self._n_ctx(pe)
        P1 = self.plan(B, h, w, steps, do_cfg, guidance_scale, lane=lane, kind="latents", n_ctx=n_ctx)
        P2 = self._from_state_plan(B, W2, H2, hr_steps, strength, guidance_scale, lane, n_ctx=n_ctx)
        for b, s in enumerate(seeds):
            l0, lo, hi = noises[b] if noises is not None else draw_noise_hires(s, h, w, steps, h2, w2, hr_steps,
                                                                               self.sched.init_noise_sigma)
            if len(lo) != steps - 1 or len(hi) != hr_steps:
                raise LcmHipError(f"request {b}: {len(lo)} + {len(hi)} noise tensors drawn ahead, the chain needs "
                                  f"{steps - 1} + {hr_steps}")
            P1.h_lat[b].copy_(l0[0])
            for i, n in enumerate(lo):
                P1.h_noise[i, b].copy_(n[0])
            for i, n in enumerate(hi):
                P2.h_noise[i, b].copy_(n[0])
        low = P1.lat[B:] if do_cfg else P1.lat
        vary = self._stage_variation(P1, variation, B, h, w)

        def front(eager):                                # stage 1 -> hand-over into stage 2's state
            self._run_plan(P1, guidance_scale, eager)
            ops.latents_upscale_renoise(low, h, w, P2.noise[0], nsa, nsb, mode, P2.lat, B, h2, w2, x_up=P2.xk[0], dup=do_cfg)

        out, _ = self._request([P1, P2], pe, negative_embeds, guidance_scale, front=front, want_float=want_float,
                               more=lambda: P1.h_latout.copy_(low, non_blocking=True), vary=vary)
        out.update(lowres_latents=P1.h_latout.numpy().copy(), unet_evals=(steps + hr_steps) * (2 if do_cfg else 1))
        if want_float:
            out["upscaled_latents"] = P2.xk[0].cpu().numpy()
        return out

    @torch.inference_mode()
    def generate(self, prompt_embeds, seeds, width, height, steps, guidance_scale=1.0, negative_embeds=None,
                 want_float=False, taps=None, latents=None, added=None, negative_added=None, noises=None, lane=0,
                 strength=None, passes=0, start=None, control=None, hires=None, preprocess=None, variation=None, sampler=None):
        """prompt_embeds: [B,77 n,ctx] (any float dtype, host or device; n chunks of a long prompt, concatenated: the
        plan, its graph and its cross-attention launches are those of n -- n = 1 is the plan of always); seeds: B ints.  noises: optional per-request
        ``draw_noise(seed, h, w, steps - 1, init_noise_sigma)`` results drawn ahead by the callers (the worker's pool
        threads draw them in parallel, off the dispatcher's serial path); None: drawn here from the seeds.
        lane: which of the pipeline's concurrent sampler instances runs the request (calls on different lanes may overlap;
        calls on one lane must be serialised by the caller).
        passes > 0: refinement in latent space -- the plain request's final latents x^0, then ``passes`` times: re-noise to
        the first timestep of ``timesteps(steps, strength)`` and run the LCM steps over that schedule; the image is the decode
        of x^passes.  A request's RNG stream is then ``draw_noise(seed, h, w, steps * (passes + 1) - 1)``: the plain request's
        tensors first, then per pass its re-noise draw and its steps - 1 step noises.  start = (k, [B device tensors fp32
        [4,h,w]]): the chain starts from these x^k (0 <= k < passes) and runs passes - k passes; the draws of the passes
        left out are skipped, so the result does not depend on where the chain started.  The result then carries
        ``xk_first`` and ``xk`` (device fp32 [n,B,4,h,w]: x^xk_first ... x^passes) and ``unet_evals``.
        control = (hint uint8 [B,H,W,3] at the request's size, conditioning_scale): ControlNet-conditioned generation with the
        ControlNet of set_controlnet.  The scale is part of the plan key (the captured GEMMs carry it as a scalar argument);
        the hint is uploaded per request into the plan's fixed buffer.  Not combined with passes.  The result then carries
        ``controlnet_evals``.
        preprocess = ("canny", low, high) | ("invert",): the hint is a photo, and its edge map (include/lcm_hip.h, Canny) or its
        inverse is computed on the lane's stream, between the upload and the captured pass, into the buffer the hint stack reads
        (csrc/canny.hip; per-lane workspace sized on first use).  It is no part of the plan key: plans, graphs and launches of
        the pass are those of a finished hint.  None / (): the hint is the finished map.  Needs control.
        hires = (W2, H2, hr_steps, strength, mode): hires fix -- ``generate_hires`` (its own RNG contract and result keys); not
        combined with passes, control, latents or SDXL conditioning.
        variation: per request None | (t, sub, base | None) -- variation seeds and seed-resize (module docstring;
        ``draw_variation``).  sub / base fp32 host tensors [1,4,hs,ws], already multiplied by init_noise_sigma; t the subseed strength
        in [0, 1].  base None: the request's own initial latents are blended in place with sub ((hs, ws) = (h, w)); with a base the
        blend happens at the source shape and is pasted, centred, into them (include/lcm_hip.h, variation seeds).  One launch of
        lcm_noise_variation_f32 for the whole batch, on the lane's stream between the uploads and the captured pass; slots with
        None are not touched, and a call without any variation queues nothing.  It is no part of the plan key.  A chain that
        starts from cached latents (start=) never reads the initial latents, so nothing is launched there.
        sampler = (name, "normal" | "karras") with name one of samplers.py's Euler, Euler a, DDIM, DPM++ 2M: the pass steps with that
        sampler (``_sampler_pass``; include/lcm_hip.h, samplers) instead of the LCM sampler.  It is part of the plan key.  The
        request draws exactly what it draws without one; Euler a reads the step noises, the others ignore them.  Combined with
        control, variation and long prompts; not with passes, hires or SDXL conditioning.
        Returns dict(rgb uint8 [B,H,W,3] (host), latents fp32 [B,4,h,w] (host), pool8 fp16 [B,4,8,8] (host))."""
        torch.cuda.set_device(self.device)        # the pool may call from a thread other than the constructing one
        if sampler is not None:
            if hires is not None or passes or start is not None or (strength is not None and float(strength) != 1.0):
                raise LcmHipError("a sampler is not combined with hires fix or refinement passes")
            if self.unet.has_added:
                raise LcmHipError("samplers are not served for SDXL-family UNets")
            if not 1 <= int(steps) <= _samplers.MAX_STEPS:
                raise LcmHipError(f"num_inference_steps={int(steps)} outside 1..{_samplers.MAX_STEPS} with a sampler")
        if hires is not None:
            if passes or start is not None or (strength is not None and float(strength) != 1.0):
                raise LcmHipError("hires fix is not combined with refinement passes")
            if control is not None:
                raise LcmHipError("hires fix is not combined with a ControlNet hint")
            if latents is not None or added is not None or taps is not None:
                raise LcmHipError("hires fix draws its noise from the seeds and is not served for SDXL: latents= / added= / taps= "
                                  "are not supported")
            return self.generate_hires(prompt_embeds, seeds, width, height, steps, hires, guidance_scale, negative_embeds,
                                       want_float=want_float, noises=noises, lane=lane, variation=variation)
        pe = torch.as_tensor(prompt_embeds)
        B = pe.shape[0]
        check_size(width, height)
        h, w = height // VAE_SCALE_FACTOR, width // VAE_SCALE_FACTOR
        steps = int(steps)
        do_cfg = self._do_cfg(guidance_scale, negative_embeds)
        if self.unet.has_added and added is None:
            raise LcmHipError("this UNet needs added=(pooled_text_embeds [B,P], time_ids [B,6]) (SDXL text_time embedding)")
        passes = int(passes or 0)
        refine, n_extra, skip = None, steps - 1, 0
        if passes > 0:
            if latents is not None:
                raise LcmHipError("refinement passes draw their noise from the seeds: latents= is not supported with passes > 0")
            k0 = int(start[0]) if start is not None else None
            if k0 is not None and not 0 <= k0 < passes:
                raise LcmHipError(f"start depth {k0} outside [0, passes={passes})")
            dd = 1.0 if strength is None else float(strength)
            self.sched.timesteps(steps, dd)           # diffusers' error for steps > original_steps x strength, before any plan
            refine = (dd, passes - (k0 or 0), k0 is not None)
            n_extra = steps * (passes + 1) - 1
            skip = steps * (k0 + 1) - 1 if k0 is not None else 0
        elif strength is not None and float(strength) != 1.0:
            raise LcmHipError("strength needs passes >= 1")
        hint = cscale = None
        if control is not None:
            if refine is not None:
                raise LcmHipError("a ControlNet hint is not combined with refinement passes")
            if self.controlnet is None:
                raise LcmHipError("this request carries a ControlNet hint but no ControlNet is loaded (set_controlnet)")
            hint, cscale = control
            cscale = float(cscale)
            if not 0.0 <= cscale <= 2.0:
                raise LcmHipError(f"controlnet conditioning scale {cscale} outside [0, 2]")
            hint, hint_fit = self._sources(hint, B, (height, width, 3), "ControlNet hint")
        pre = tuple(preprocess) if preprocess else ()
        if pre:
            if control is None:
                raise LcmHipError("a ControlNet preprocessor needs a hint to work on (control=)")
            if not ((pre[0] == "canny" and len(pre) == 3) or pre == ("invert",)):
                raise LcmHipError(f"unknown ControlNet preprocessor {pre!r}: expected ('canny', low, high) or ('invert',)")
        P = self.plan(B, h, w, steps, do_cfg, guidance_scale, lane=lane, refine=refine, control=cscale, n_ctx=self._n_ctx(pe),
                      sampler=sampler)
        with torch.cuda.stream(P.lane.stream):       # latents= and the hint may be device tensors
            for b, s in enumerate(seeds):
                if latents is not None:
                    P.h_lat[b].copy_(torch.as_tensor(latents[b]).reshape(4, h, w))
                    extra = []
                else:
                    l0, extra = noises[b] if noises is not None else draw_noise(s, h, w, n_extra, self.sched.init_noise_sigma)
                    if refine is not None:
                        if len(extra) != n_extra:
                            raise LcmHipError(f"request {b}: {len(extra)} noise tensors drawn ahead, the chain needs {n_extra}")
                        extra = extra[skip:]
                    P.h_lat[b].copy_(l0[0])
                for i, n in enumerate(extra):
                    P.h_noise[i, b].copy_(n[0])
            if hint is not None:
                self._stage(P.h_hint, hint)
        vary = None
        if variation is not None and not (refine is not None and refine[2]):
            if self.unet.has_added:
                raise LcmHipError("variation seeds are not served for SDXL-family UNets")
            vary = self._stage_variation(P, variation, B, h, w)

        def upload():
            if hint is not None:
                P.hint.copy_(P.h_hint, non_blocking=True)
                self._fit_pending(P.lane, hint_fit, P.hint)      # a photo or map of another size: fitted ahead of the preprocessor
                if pre:
                    self._preprocess_hint(P, pre, B, height, width)
            if refine is not None and refine[2]:
                for b in range(B):
                    P.xk[0, b].copy_(start[1][b].reshape(4, h, w), non_blocking=True)
            if self.unet.has_added:
                self._upload_added(P, added, negative_added)

        out, xk = self._request([P], pe, negative_embeds, guidance_scale, upload, want_float=want_float, taps=taps,
                                more=(lambda: P.xk.clone()) if refine is not None else None, vary=vary)
        if refine is not None:
            out["xk"], out["xk_first"] = xk, passes - refine[1]
            out["unet_evals"] = steps * (refine[1] + (0 if refine[2] else 1))
        if control is not None:
            out["controlnet_evals"] = steps
        return out

    @staticmethod
    def _sources(pics, B, shape, what):
        """The per-request uploads of a batch -> (host pictures, device fits).  pics: uint8 [B] + shape (array or tensor: every
        picture at the request's size, the usual call), or a list of B entries, each a uint8 array of ``shape`` or a
        ``backends.fit.Pending`` -- a picture of another size that the lane's stream is to fit (LCM_RESIZE=hip).  -> (one tensor
        [B] + shape, None), or ([B tensors | None], [B Pending | None])."""
        from .backends.fit import Pending
        if isinstance(pics, (list, tuple)) and any(isinstance(p, Pending) for p in pics):
            if len(pics) != B:
                raise LcmHipError(f"{what}: {len(pics)} entries for a batch of {B}")
            host, fits = [], []
            for p in pics:
                if isinstance(p, Pending):
                    a = p.pixels
                    if (a.dtype != np.uint8 or a.ndim != len(shape) or a.shape[2:] != tuple(shape[2:]) or (p.height, p.width) != tuple(shape[:2])
                            or min(a.shape) < 1):
                        raise LcmHipError(f"{what}: a picture to fit must be uint8 [h, w{', 3' if len(shape) == 3 else ''}] for a "
                                          f"{shape[1]}x{shape[0]} request, got {a.dtype} {tuple(a.shape)} for {p.width}x{p.height}")
                    host.append(None), fits.append(p)
                else:
                    t = torch.as_tensor(p)
                    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape):
                        raise LcmHipError(f"{what} must be uint8 {list(shape)}, got {t.dtype} {tuple(t.shape)}")
                    host.append(t), fits.append(None)
            return host, fits
        try:
            t = torch.stack([torch.as_tensor(p) for p in pics]) if isinstance(pics, (list, tuple)) else torch.as_tensor(pics)
        except (RuntimeError, TypeError, ValueError) as e:
            raise LcmHipError(f"{what} must be uint8 {[B] + list(shape)}: {e}")
        if t.dtype != torch.uint8 or tuple(t.shape) != (B,) + tuple(shape):
            dims = ", ".join(f"{n}={v}" for n, v in zip("HW", shape[:2])) + (", 3" if len(shape) == 3 else "")
            raise LcmHipError(f"{what} must be uint8 [B={B}, {dims}], got {t.dtype} {tuple(t.shape)}")
        return t, None

    @staticmethod
    def _stage(h_buf, host):
        """Fill the pinned staging of a batch of uploads: the whole batch, or the slots that came at the request's size."""
        if isinstance(host, list):
            for b, t in enumerate(host):
                if t is not None:
                    h_buf[b].copy_(t)
        else:
            h_buf.copy_(host)

    def _fit_pending(self, L: _Lane, fits, dst):
        """The uploads that came at another size, on the current (the lane's) stream, outside any captured graph: per picture the
        raw upload into the lane's source buffer, then the Lanczos resampler (include/lcm_hip.h; csrc/resize.hip) straight into
        slot b of dst ([B,H,W,3] or [B,H,W]).  Source buffer and workspace belong to the lane and grow on demand; they are
        allocated on this stream, which orders every reuse behind the launches that read them.  Nothing is read back.
        Neighbouring entries that hold the same ``pixels`` object (the tiles of an SD-upscale request: windows of one grid of
        one picture) share one upload: the source buffer still holds it."""
        if not fits:
            return
        held = None                                      # the pixels object L.fit_src holds
        for b, f in enumerate(fits):
            if f is None:
                continue
            a = torch.from_numpy(f.pixels)
            n = a.numel()
            if L.fit_src is None or L.fit_src.numel() < n:
                L.fit_src = torch.empty(n, dtype=torch.uint8, device=self.device)
                held = None
            src = L.fit_src[:n].view(a.shape)
            if f.pixels is not held:
                src.copy_(a, non_blocking=True)
                held = f.pixels
            sh, sw = a.shape[:2]
            win = (f.x0, f.y0, f.width, f.height)
            need = ops.resize_ws_bytes(sw, sh, 1 if a.dim() == 2 else 3, f.fit_w, f.fit_h, win)
            if need <= 0:
                raise LcmHipError(f"a {sw}x{sh} picture fitted to {f.fit_w}x{f.fit_h} is outside the resampler's domain")
            if L.fit_ws is None or L.fit_ws.numel() < need:
                L.fit_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            ops.resize_lanczos_u8(src, dst[b], L.fit_ws, f.fit_w, f.fit_h, win)

    def grid_store(self, lane, n_tiles, tile_h, tile_w):
        """The lane's tile store of an SD-upscale request: uint8 [n_tiles, tile_h, tile_w, 3] on the device, a view of a buffer
        that belongs to the lane, grows on demand and is allocated on the lane's stream (like the resampler's source buffer:
        every reuse is ordered behind the launches that read it).  ``generate_img2img(tiles=)`` fills it pass by pass."""
        L = self.lane(lane)
        n = int(n_tiles) * int(tile_h) * int(tile_w) * 3
        if not 0 < n < 1 << 31:
            raise LcmHipError(f"{n_tiles} tiles of {tile_w}x{tile_h} are outside the combine launch's domain (2^31 bytes)")
        if L.grid_tiles is None or L.grid_tiles.numel() < n:
            with torch.cuda.stream(L.stream):
                L.grid_tiles = torch.empty(n, dtype=torch.uint8, device=self.device)
        return L.grid_tiles[:n].view(int(n_tiles), int(tile_h), int(tile_w), 3)

    @torch.inference_mode()
    def combine_grid(self, lane, store, W, H, overlap, xs, ys):
        """The tiles of ``store`` (``grid_store``; tile r * cols + c at (xs[c], ys[r])) -> the W x H picture, uint8 [H, W, 3] on
        the host: one launch of lcm_grid_combine_rgb8 on the lane's stream (include/lcm_hip.h defines the bytes), one
        device-to-host copy, one synchronize.  No tile pixel travels to the host for it."""
        torch.cuda.set_device(self.device)
        L = self.lane(lane)
        th, tw = int(store.shape[1]), int(store.shape[2])
        desc = ops.grid_desc(W, H, tw, th, overlap, xs, ys)
        if store.shape[0] != desc.rows * desc.cols:
            raise LcmHipError(f"a grid of {desc.cols} x {desc.rows} tiles and a store of {store.shape[0]}")
        n = int(W) * int(H) * 3
        with torch.cuda.stream(L.stream):
            if L.grid_out is None or L.grid_out.numel() < n:
                L.grid_out = torch.empty(n, dtype=torch.uint8, device=self.device)
                L.h_grid = torch.empty(n, dtype=torch.uint8).pin_memory()
            out, host = L.grid_out[:n], L.h_grid[:n]
            ops.grid_combine_rgb8(store, out, desc)
            host.copy_(out, non_blocking=True)
            L.stream.synchronize()
        return host.numpy().reshape(int(H), int(W), 3).copy()

    def _stage_variation(self, P: _Plan, variation, B, h, w):
        """The variations of a batch (``generate``'s variation=) -> None when no slot has one, else vary(): called on the lane's
        stream after the uploads, it copies the staged sub / base tensors to the device and queues the one launch of
        lcm_noise_variation_f32 into P.lat0.  Here, on the caller's side and before anything is launched, the tensors are checked
        and copied into the lane's pinned staging.  Pinned and device staging belong to the lane, are sized on first use and grow
        on demand (a lane that never sees a variation owns neither); the device side is allocated on the lane's stream, which
        orders every reuse behind the launch that read it.  Nothing is read back."""
        if variation is None:
            return None
        if len(variation) != B:
            raise LcmHipError(f"variation: {len(variation)} entries for a batch of {B}")
        slots, n = [], 0                                 # per slot None | (t, hs, ws, offset of sub | None, offset of base | None)
        srcs = []
        for b, v in enumerate(variation):
            if v is None:
                slots.append(None)
                continue
            t, sub, base = v
            t = float(t)
            if not 0.0 <= t <= 1.0:                      # NaN fails both comparisons
                raise LcmHipError(f"request {b}: variation strength {t} outside [0, 1]")
            if t > 0.0 and sub is None:
                raise LcmHipError(f"request {b}: a variation of strength {t} needs the subseed's noise")
            if t == 0.0 and base is None:                # nothing to blend, nothing to paste: the plain request
                slots.append(None)
                continue
            ts = [None if x is None else torch.as_tensor(x, dtype=torch.float32).reshape(-1, *torch.as_tensor(x).shape[-2:])
                  for x in ((sub if t > 0.0 else None), base)]
            shape = next(x.shape for x in ts if x is not None)
            hs, ws = int(shape[1]), int(shape[2])
            if any(x is not None and tuple(x.shape) != (4, hs, ws) for x in ts) or not (1 <= hs <= 256 and 1 <= ws <= 256):
                raise LcmHipError(f"request {b}: variation noise must be fp32 [1,4,hs,ws] with sides in 1..256, got "
                                  f"{[None if x is None else tuple(x.shape) for x in ts]}")
            if base is None and (hs, ws) != (h, w):
                raise LcmHipError(f"request {b}: a variation without a seed-resize base blends in place and needs noise of the "
                                  f"request's latent shape {h}x{w}, got {hs}x{ws}")
            offs = []
            for x in ts:
                offs.append(None if x is None else n)
                if x is not None:
                    srcs.append((n, x))
                    n += x.numel()
            slots.append((t, hs, ws, offs[0], offs[1]))
        if n == 0:
            return None
        L = P.lane
        if L.var_h is None or L.var_h.numel() < n:
            L.var_h = torch.empty(n, dtype=torch.float32).pin_memory()
        for o, x in srcs:
            L.var_h[o:o + x.numel()].copy_(x.reshape(-1))

        def vary():
            if L.var_d is None or L.var_d.numel() < n:
                L.var_d = torch.empty(L.var_h.numel(), dtype=torch.float32, device=self.device)
            L.var_d[:n].copy_(L.var_h[:n], non_blocking=True)
            view = lambda o, hs, ws: None if o is None else L.var_d[o:o + 4 * hs * ws]
            # low: the seed-resize base, or None -- the slot itself, blended in place
            ops.noise_variation(P.lat0, B, h, w, [None if s is None else (view(s[4], s[1], s[2]), view(s[3], s[1], s[2]), s[1], s[2], s[0])
                                                  for s in slots])
        return vary

    def _preprocess_hint(self, P: _Plan, pre, B, H, W):
        """The photo in P.hint (uploaded, and fitted where it came at another size) -> the map in P.hint, on the current (the
        lane's) stream: the preprocessor's launches in place (the picture is read by the first launch only, the map written by
        the last).  Nothing is read back."""
        if pre[0] == "invert":
            ops.invert_u8(P.hint, P.hint)
            return
        L = P.lane
        need = ops.canny_ws_bytes(B, H, W)
        if L.pre_ws is None or L.pre_ws.numel() < need:
            L.pre_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        ops.canny_rgb8(P.hint, P.hint, L.pre_ws, B, H, W, float(pre[1]), float(pre[2]))

    # hot loop only (device resident inputs already in the plan): used by bench.py
    def replay(self, P: _Plan):
        if P.graph is None:
            raise LcmHipError("plan has no captured graph")
        P.graph.launch()
