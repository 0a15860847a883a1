"""The ControlNet preprocessors on the MI355X (csrc/canny.hip) against tests/canny_reference.py.  Everything is integer
arithmetic defined bit for bit by include/lcm_hip.h, so every comparison here is for equality: the class map of the stencil
stage, the edge picture of the link stage on designed class maps (spirals that need thousands of growth rounds), the composed
call, determinism, and the worker's ``controlnet_module`` against the same request carrying the reference's map as a finished
hint."""
import io
import os
from dataclasses import dataclass, field
from typing import Any, Optional

import numpy as np
import pytest
import torch

import canny_reference as cy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _classes(imgs, lo, hi):
    """uint8 [B,H,W,3] host -> the device's class map, uint8 [B,H,W] host."""
    from sdlcm_amd import ops
    B, H, W = imgs.shape[:3]
    out = torch.full((B, H, W), 77, dtype=torch.uint8, device=DEV)
    ops.canny_classes(_dev(imgs), out, B, H, W, lo, hi)
    return out.cpu().numpy()


def _link(cls):
    """uint8 [B,H,W] host class maps -> the device's edge picture, uint8 [B,H,W,3] host."""
    from sdlcm_amd import ops
    B, H, W = cls.shape
    ws = torch.full((ops.canny_ws_bytes(B, H, W),), 0xA5, dtype=torch.uint8, device=DEV)      # poisoned: nothing relies on zeros
    out = torch.full((B, H, W, 3), 77, dtype=torch.uint8, device=DEV)
    ops.canny_link(_dev(cls), out, ws, B, H, W)
    return out.cpu().numpy()


def _canny(imgs, low, high, stream=None):
    from sdlcm_amd import ops
    B, H, W = imgs.shape[:3]
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        ws = torch.full((ops.canny_ws_bytes(B, H, W),), 0x5A, dtype=torch.uint8, device=DEV)
        out = torch.full((B, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        ops.canny_rgb8(_dev(imgs), out, ws, B, H, W, low, high)
        host = out.cpu()
    return host.numpy()


def _ref_classes(imgs, lo, hi):
    return np.stack([cy.classes(i, lo, hi) for i in imgs])


NOISE_SHAPES = [(64, 64), (40, 72), (136, 264)]


@pytest.fixture(scope="module")
def noise():
    """The smoothed-noise pictures and their reference results, computed once."""
    pics = {hw: cy.smoothed_noise(hw[0], hw[1], seed=10 + i) for i, hw in enumerate(NOISE_SHAPES)}
    pics["batch"] = np.stack([cy.smoothed_noise(24, 40, seed=50 + b, passes=2 + b % 4) for b in range(8)])
    return pics


# ---- the classes stage ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", NOISE_SHAPES)
@pytest.mark.parametrize("lo,hi", [(100, 200), (20, 60), (5, 400)])
def test_classes_noise(noise, hw, lo, hi):
    img = noise[hw][None]
    got, want = _classes(img, lo, hi), _ref_classes(img, lo, hi)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} classes differ"
    assert (want == 1).any() or (want == 2).any()


def test_classes_batch_of_eight(noise):
    imgs = noise["batch"]
    for lo, hi in ((100, 200), (5, 400)):
        got, want = _classes(imgs, lo, hi), _ref_classes(imgs, lo, hi)
        assert np.array_equal(got, want)
    assert len({w.tobytes() for w in want}) == 8


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (3, 5), (8, 33), (9, 32), (17, 65)])
def test_classes_degenerate_sizes(h, w):
    g = np.random.default_rng(h * 100 + w)
    img = g.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    for lo, hi in ((1, 2), (100, 200), (600, 1200)):
        assert np.array_equal(_classes(img, lo, hi), _ref_classes(img, lo, hi)), (h, w, lo, hi)


def _designed():
    g = np.random.default_rng(3)
    step = np.zeros((8, 8, 3), np.uint8)
    step[:, 4:] = 255
    extremes = (g.integers(0, 2, (40, 72, 3)) * 255).astype(np.uint8)            # magnitudes up to the maximum, 1530
    blocks = np.repeat(np.repeat((g.integers(0, 4, (10, 18, 3)) * 85).astype(np.uint8), 4, axis=0), 4, axis=1)   # 4 x 4 flat blocks
    gray = np.repeat(cy.smoothed_noise(40, 72, 8)[..., :1], 3, axis=2)
    ch2 = np.zeros((40, 72, 3), np.uint8)
    ch2[..., 2] = cy.smoothed_noise(40, 72, 9)[..., 0]
    ch2[..., 0] = ch2[..., 2] // 4
    checker = np.repeat((((np.add.outer(np.arange(33), np.arange(35))) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    return dict(step=step, step_t=np.ascontiguousarray(step.transpose(1, 0, 2)), extremes=extremes, blocks=blocks, gray=gray, ch2=ch2,
                black=np.zeros((19, 37, 3), np.uint8), white=np.full((19, 37, 3), 255, np.uint8), checker=checker)


@pytest.mark.parametrize("name", sorted(_designed()))
def test_classes_designed_pictures(name):
    img = _designed()[name][None]
    for lo, hi in ((100, 200), (1, 255), (100, 1019), (100, 1020), (1020, 1020), (1529, 1530), (1528, 1529)):
        got, want = _classes(img, lo, hi), _ref_classes(img, lo, hi)
        assert np.array_equal(got, want), (name, lo, hi, int((got != want).sum()))


def test_classes_designed_pictures_say_what_they_should():
    d = _designed()
    # the largest magnitude there is: dx and dy share the corner pixels with opposite signs, so |dx| + |dy| <= 6 * 255
    assert cy.gradients(d["extremes"])[2].max() == 1530
    assert np.all(_classes(d["step"][None], 100, 1019)[0][:, 3] == 2)
    assert np.all(_classes(d["step"][None], 100, 1020)[0][:, 3] == 1)
    assert not _classes(d["step"][None], 1020, 1020).any()
    assert not _classes(d["black"][None], 0, 0).any()
    m = cy.gradients(d["ch2"])
    one = np.zeros_like(d["ch2"])
    one[..., 2] = d["ch2"][..., 2]
    assert np.array_equal(cy.gradients(one)[2], m[2])                             # channel 2 decides everywhere
    assert np.array_equal(_classes(d["step"][None], 200, 100), _classes(d["step"][None], 100, 200))   # swapped thresholds


# ---- the link stage on designed class maps -------------------------------------------------------------------------------------
def _check_link(cls):
    got = _link(cls)
    want = cy.link_rgb(cls)
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).any(axis=-1).sum())} pixels differ"
    return got


@pytest.mark.parametrize("h,w", [(64, 64), (40, 72)])
def test_link_spiral(h, w):
    s = cy.spiral(h, w)
    got = _check_link(s[None])
    assert np.array_equal(got[0, ..., 0] == 255, s > 0)                           # the whole spiral hangs on its inner end
    assert not _check_link(cy.spiral(h, w, strong=False)[None]).any()
    # the strong pixel at the outer end instead, and in the middle of the chain
    t = cy.spiral(h, w, strong=False)
    t[0, 0] = 2
    _check_link(t[None])


def test_link_spiral_batch_does_not_leak():
    s = np.stack([cy.spiral(64, 64), cy.spiral(64, 64, strong=False)])
    got = _check_link(s)
    assert got[0].any() and not got[1].any()
    got = _check_link(s[::-1].copy())
    assert got[1].any() and not got[0].any()


def test_link_designed_maps():
    diag = np.zeros((2, 70, 70), np.uint8)                                         # two bars that touch only diagonally, across a tile corner
    diag[0, 10:32, 31], diag[0, 32:50, 32] = 1, 1
    diag[0, 49, 32] = 2
    diag[1, 10:32, 32], diag[1, 32:50, 31] = 1, 1                                  # the other diagonal
    diag[1, 10, 32] = 2
    _check_link(diag)
    gap = diag.copy()
    gap[0, 32, 32] = 0                                                             # one pixel out: the far bar is no edge
    got = _check_link(gap)
    assert not got[0, 10:32, 31].any()
    g = np.random.default_rng(11)
    strong_only = (g.random((1, 40, 72)) < 0.3).astype(np.uint8) * 2
    _check_link(strong_only)
    frame = np.ones((1, 40, 72), np.uint8)
    frame[0, -1, -1] = 2
    assert _check_link(frame).all()
    assert not _check_link(np.ones((1, 40, 72), np.uint8)).any()
    assert not _check_link(np.zeros((1, 40, 72), np.uint8)).any()
    rnd = g.choice(np.array([0, 1, 2], np.uint8), size=(3, 70, 99), p=[0.55, 0.44, 0.01])    # percolating weak clusters, few seeds
    _check_link(rnd)
    for h, w in ((1, 1), (1, 9), (9, 1), (3, 5), (33, 31)):
        _check_link(g.choice(np.array([0, 1, 2], np.uint8), size=(2, h, w), p=[0.4, 0.5, 0.1]))


# ---- the composed call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", NOISE_SHAPES)
def test_composed_noise(noise, hw):
    img = noise[hw]
    for low, high in ((100, 200), (20, 60), (5, 400), (200, 100), (100.9, 200.9)):
        got, want = _canny(img[None], low, high)[0], cy.canny(img, low, high)
        assert np.array_equal(got, want), (hw, low, high, int((got != want).any(axis=-1).sum()))
    if hw == (64, 64):
        c = cy.classes(img, 5, 400)
        assert cy.growth_rounds(c) > 8 and (c == 1).sum() > 20 * (c == 2).sum() > 0           # hysteresis has real work here


def test_composed_batch_small_and_in_place(noise):
    from sdlcm_amd import ops
    imgs = noise["batch"]
    want = cy.canny(imgs, 5, 400)
    assert np.array_equal(_canny(imgs, 5, 400), want)
    for b in (0, 5):
        assert np.array_equal(_canny(imgs[b:b + 1], 5, 400)[0], want[b])
    x = _dev(imgs)
    ws = torch.empty(ops.canny_ws_bytes(*imgs.shape[:3]), dtype=torch.uint8, device=DEV)
    ops.canny_rgb8(x, x, ws, *imgs.shape[:3], 5, 400)
    assert np.array_equal(x.cpu().numpy(), want)
    assert not _canny(np.full((1, 1, 1, 3), 9, np.uint8), 100, 200).any()
    step = _designed()["step"]
    e = _canny(step[None], 100, 200)[0]
    assert np.array_equal(np.nonzero(e[..., 0])[1], np.full(8, 3)) and int((e[..., 0] == 255).sum()) == 8
    assert not _canny(step[None], 100, 1020).any()


def test_invert_and_host_helper(noise):
    from sdlcm_amd import ops
    from sdlcm_amd.backends.hip_worker import canny
    for n in (1, 15, 16, 17, 4099):
        a = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
        out = torch.zeros(n, dtype=torch.uint8, device=DEV)
        ops.invert_u8(_dev(a), out)
        assert np.array_equal(out.cpu().numpy(), 255 - a)
    big = torch.arange(4100, dtype=torch.int32, device=DEV).to(torch.uint8)
    view = big[1:]                                                                 # an unaligned pointer
    ops.invert_u8(view, view)
    assert np.array_equal(view.cpu().numpy(), 255 - (np.arange(1, 4100) % 256).astype(np.uint8))
    img = noise[(40, 72)]
    assert np.array_equal(canny(img), cy.canny(img, 100, 200))
    assert np.array_equal(canny(noise["batch"], 20, 60), cy.canny(noise["batch"], 20, 60))
    with pytest.raises(ValueError):
        canny(img.astype(np.float32))


def test_errors_before_anything_is_enqueued():
    from sdlcm_amd import lib, ops
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(ops.canny_ws_bytes(1, 8, 8), dtype=torch.uint8, device=DEV)
    assert ops.canny_ws_bytes(1, 8, 8) >= 64 + 8 * 64 and ops.canny_ws_bytes(0, 8, 8) == 0
    with pytest.raises(lib.LcmHipError, match="workspace"):
        ops.canny_rgb8(x, x, ws[:100], 1, 8, 8)
    with pytest.raises(lib.LcmHipError, match="shape"):
        ops.canny_rgb8(x, x, ws, 1, 0, 8)
    with pytest.raises(lib.LcmHipError, match="thresholds"):
        ops.canny_rgb8(x, x, ws, 1, 8, 8, float("nan"), 200)
    with pytest.raises(lib.LcmHipError, match="overlaps"):
        ops.canny_rgb8(x, ws, ws, 1, 8, 8)
    with pytest.raises(lib.LcmHipError, match="null"):
        ops.canny_classes(x, None, 1, 8, 8, 1, 2)


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_determinism_streams_and_batch(noise):
    img = noise[(136, 264)]
    first = _canny(img[None], 5, 400)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    for s in (None, s1, s2, s1):
        assert np.array_equal(_canny(img[None], 5, 400, stream=s), first)
    spirals = np.stack([cy.spiral(64, 64), cy.spiral(64, 64, strong=False), cy.spiral(64, 64)])
    a = _link(spirals)
    for _ in range(3):
        assert np.array_equal(_link(spirals), a)
    imgs = noise["batch"]
    whole = _canny(imgs, 20, 60)
    for b in range(8):
        assert np.array_equal(_canny(imgs[b:b + 1], 20, 60)[0], whole[b]), b


def test_pipeline_preprocess_equals_finished_map_on_either_lane(noise):
    """generate(preprocess=) gives the bytes of the same call with the reference's map as the hint: solo, on lane 0 and lane 1, in
    a batch of 4 with different photos; a finished-hint call in between keeps its bytes."""
    from sdlcm_amd import weights
    from sdlcm_amd.lib import LcmHipError
    from sdlcm_amd.pipeline import LcmHipPipeline
    pe = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16)
    p = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device=DEV)
    try:
        p.set_controlnet(weights.synthetic_controlnet())
        photos = np.stack([cy.smoothed_noise(64, 64, 70 + b) for b in range(4)])
        maps = cy.canny(photos, 5, 400)
        assert maps.any() and len({m.tobytes() for m in maps}) == 4
        want = p.generate(pe, [42], 64, 64, 2, 1.0, control=(maps[:1], 1.0))["rgb"].copy()
        as_photo = p.generate(pe, [42], 64, 64, 2, 1.0, control=(photos[:1], 1.0))["rgb"].copy()
        assert not np.array_equal(want, as_photo)
        for lane in (0, 1, 0):
            got = p.generate(pe, [42], 64, 64, 2, 1.0, control=(photos[:1], 1.0), preprocess=("canny", 5, 400), lane=lane)
            assert np.array_equal(got["rgb"], want), f"lane {lane}"
            assert got["controlnet_evals"] == 2
        assert np.array_equal(p.generate(pe, [42], 64, 64, 2, 1.0, control=(maps[:1], 1.0))["rgb"], want)
        inv = p.generate(pe, [42], 64, 64, 2, 1.0, control=(photos[:1], 1.0), preprocess=("invert",))["rgb"]
        assert np.array_equal(inv, p.generate(pe, [42], 64, 64, 2, 1.0, control=(255 - photos[:1], 1.0))["rgb"])
        pe4 = pe.expand(4, -1, -1).contiguous()
        seeds = [42, 43, 44, 45]
        b4 = p.generate(pe4, seeds, 64, 64, 2, 1.0, control=(photos, 1.0), preprocess=("canny", 5, 400))["rgb"]
        assert np.array_equal(b4, p.generate(pe4, seeds, 64, 64, 2, 1.0, control=(maps, 1.0))["rgb"])
        assert np.array_equal(b4[0], want[0])
        with pytest.raises(LcmHipError, match="preprocessor"):
            p.generate(pe, [42], 64, 64, 2, 1.0, preprocess=("canny", 5, 400))
        with pytest.raises(LcmHipError, match="preprocessor"):
            p.generate(pe, [42], 64, 64, 2, 1.0, control=(photos[:1], 1.0), preprocess=("depth",))
    finally:
        p.close()


# ---- the worker ------------------------------------------------------------------------------------------------------------------
@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str
    size: str = "64x64"
    num_inference_steps: int = 2
    guidance_scale: float = 1.0
    seed: Optional[int] = None
    style_lora: _Style = field(default_factory=_Style)
    controlnet_image: Any = None
    controlnet_conditioning_scale: Optional[float] = None
    controlnet_module: Any = None
    controlnet_threshold_a: Any = None
    controlnet_threshold_b: Any = None


@dataclass
class _Job:
    req: _Req


def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr, "RGB").save(b, "PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def worker():
    old = {k: os.environ.get(k) for k in ("MODEL", "MODEL_ROOT", "CONTROLNET")}
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    os.environ["CONTROLNET"] = "synthetic"
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    yield w
    w.close()
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def test_worker_module_equals_finished_hint(worker):
    from sdlcm_amd.backends import controlnet as cnb
    eng = worker._engine
    photo = cy.smoothed_noise(64, 64, 91)
    mk = lambda img, **kw: _Job(_Req(prompt="a lighthouse at dusk", seed=7, controlnet_image=img, **kw))
    plain = _Job(_Req(prompt="a lighthouse at dusk", seed=7))
    plain0 = worker.run_job(plain)
    as_hint0 = worker.run_job(mk(photo))                                           # the photo as a finished hint: today's request
    n0 = dict(eng.stats)
    # canny, default thresholds and given ones
    for kw, (lo, hi) in ((dict(), (100, 200)), (dict(controlnet_threshold_a=5, controlnet_threshold_b=255), (5, 255)),
                         (dict(controlnet_threshold_a=60.5, controlnet_threshold_b=20), (20, 60))):
        edge = cy.canny(photo, lo, hi)
        assert edge.any()
        got = worker.run_job(mk(photo, controlnet_module="canny", **kw))
        assert got == worker.run_job(mk(edge)), (lo, hi)
        assert got != as_hint0 and got[0][:8] == b"\x89PNG\r\n\x1a\n" and got[1] == 7
    assert eng.stats["controlnet_preprocessed"] - n0["controlnet_preprocessed"] == 3
    assert eng.stats["controlnet_evals"] - n0["controlnet_evals"] == 12
    assert worker.run_job(mk(_png(photo), controlnet_module="canny")) == worker.run_job(mk(cy.canny(photo, 100, 200)))
    # invert
    assert worker.run_job(mk(photo, controlnet_module="invert")) == worker.run_job(mk(255 - photo))
    assert eng.stats["controlnet_preprocessed"] - n0["controlnet_preprocessed"] == 5
    # a photo of another size goes through fit_hint first
    big = cy.smoothed_noise(96, 128, 92)
    fitted = cnb.fit_hint(big, 64, 64)
    assert fitted.shape == (64, 64, 3)
    assert worker.run_job(mk(big, controlnet_module="canny", controlnet_threshold_a=20, controlnet_threshold_b=60)) == \
        worker.run_job(mk(cy.canny(fitted, 20, 60)))
    # the scale still counts, "none" is no module, and the untouched paths keep their bytes
    half = worker.run_job(mk(photo, controlnet_module="canny", controlnet_conditioning_scale=0.5))
    assert half == worker.run_job(mk(cy.canny(photo, 100, 200), controlnet_conditioning_scale=0.5))
    n1 = eng.stats["controlnet_preprocessed"]
    assert worker.run_job(mk(photo, controlnet_module="none")) == as_hint0 and worker.run_job(mk(photo)) == as_hint0
    assert worker.run_job(plain) == plain0
    assert eng.stats["controlnet_preprocessed"] == n1
    for bad, word in ((dict(controlnet_module="depth"), "controlnet_module"),
                      (dict(controlnet_module="canny", controlnet_threshold_a=0), "controlnet_threshold_a")):
        with pytest.raises(RuntimeError, match=word):
            worker.run_job(mk(photo, **bad))
    with pytest.raises(RuntimeError, match="controlnet_image"):
        worker.run_job(_Job(_Req(prompt="p", seed=1, controlnet_module="canny")))
    assert worker.run_job(plain) == plain0


def test_worker_pool_bad_module_fails_alone(worker):
    """Through the pool-shaped loop: canny, invert, finished-hint and plain jobs drained together each get their solo bytes, and
    a bad module among them fails only its own job."""
    from test_refine_gpu import _held_pool, _minipool, _outcome
    minipool = _minipool()

    def mk(s):
        photo = cy.smoothed_noise(64, 64, 200 + s)
        extra = [dict(), dict(controlnet_image=photo), dict(controlnet_image=photo, controlnet_module="canny"),
                 dict(controlnet_image=photo, controlnet_module="invert"),
                 dict(controlnet_image=photo, controlnet_module="canny", controlnet_threshold_a=20, controlnet_threshold_b=60)][s % 5]
        return _Req(prompt=f"mixed {s}", seed=s, **extra)
    solo = {s: worker.run_job(_Job(mk(s))) for s in range(10)}
    assert solo[2] == worker.run_job(_Job(_Req(prompt="mixed 2", seed=2, controlnet_image=cy.canny(cy.smoothed_noise(64, 64, 202)))))
    pool, gate, hold = _held_pool(worker, minipool)
    try:
        n0 = len(worker._engine.batcher.batches)
        futs = [pool.submit_job(minipool.GenerationJob(req=mk(s))) for s in range(10)]
        bad = pool.submit_job(minipool.GenerationJob(req=_Req(prompt="bad", seed=99, controlnet_image=cy.smoothed_noise(64, 64, 1),
                                                              controlnet_module="lineart")))
        gate.set()
        hold.result(60)
        res = [_outcome(f) for f in futs]
        rb = _outcome(bad)
        pool.q.join()
        assert res == [solo[s] for s in range(10)]
        assert isinstance(rb, RuntimeError) and "controlnet_module" in str(rb)
        assert len(worker._engine.batcher.batches[n0:]) < 10                      # coalesced, each class among itself
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()
