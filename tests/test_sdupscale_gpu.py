"""SD upscale on the GPU: the combine launch against the integer definition (tests/sdupscale_reference.py), its refusals, and the
request end to end on the synthetic worker -- its picture against A1111's paste of the PNGs that the same worker returns for the
tiles as ordinary image-to-image requests.  Everything is exact equality."""
import ctypes as C
import io
import os
import sys
import threading
import types

import numpy as np
import pytest
import torch

import sdupscale_reference as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0xA5


def _pic(h, w, seed=0):
    """A smooth picture with some texture (seeded), uint8 [h, w, 3]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 7.0 + seed), 128 + 100 * np.cos(y / 5.0), 128 + 90 * np.sin((x + y) / 9.0)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def _decode(png):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _launch(tiles, W, H, tw, th, ov, xs, ys):
    """-> (output [H, W, 3], guard row [W, 3]) of one launch into a sentinel-filled buffer of H + 1 rows."""
    from sdlcm_amd import ops
    buf = torch.full((H + 1, W, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    ops.grid_combine_rgb8(torch.from_numpy(tiles).to(DEV), buf, (W, H, tw, th, ov, xs, ys))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return host[:H], host[H]


KERNEL_GEOMETRIES = sr.GEOMETRIES + [(128, 96, 64, 64, 0)]


@pytest.mark.parametrize("geo", KERNEL_GEOMETRIES, ids=["x".join(map(str, g)) for g in KERNEL_GEOMETRIES])
def test_kernel_equals_the_integer_definition(geo):
    W, H, tw, th, ov = geo
    xs, ys = sr.geometry(*geo)
    T = len(xs) * len(ys)
    cases = {"random": sr.random_tiles(*geo, seed=W + 3 * H + ov), "zeros": np.zeros((T, th, tw, 3), np.uint8),
             "all 255": np.full((T, th, tw, 3), 255, np.uint8)}
    for tag, tiles in cases.items():
        got, guard = _launch(tiles, W, H, tw, th, ov, xs, ys)
        want = sr.combine_int(tiles, W, H, ov, xs, ys)
        assert np.array_equal(got, want), (tag, int((got != want).sum()))
        assert (guard == SENTINEL).all(), f"{tag}: the row behind the output was written"
    assert (sr.combine_int(cases["all 255"], W, H, ov, xs, ys) == 255).all()     # blends of equal values keep them


def test_a_larger_store_and_the_capturable_call():
    """The worker's store is the head of a larger buffer; the launch inside a captured graph gives the same bytes."""
    from sdlcm_amd import ops
    geo = (104, 88, 64, 64, 40)
    W, H, tw, th, ov = geo
    xs, ys = sr.geometry(*geo)
    tiles = sr.random_tiles(*geo, seed=11)
    want = sr.combine_int(tiles, W, H, ov, xs, ys)
    store = torch.full((len(tiles) + 2, th, tw, 3), 7, dtype=torch.uint8, device=DEV)
    store[:len(tiles)] = torch.from_numpy(tiles).to(DEV)
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    desc = ops.grid_desc(W, H, tw, th, ov, xs, ys)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        ops.grid_combine_rgb8(store, out, desc)
        stream.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
        out.zero_()
        g = ops.Graph()
        with g:
            ops.grid_combine_rgb8(store, out, desc)
        g.launch()
        stream.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def _desc(**kw):
    from sdlcm_amd import ops
    d = ops.grid_desc(160, 112, 64, 64, 16, [0, 48, 96], [0, 48])
    for k, v in kw.items():
        if k in ("xs", "ys"):
            for i, x in enumerate(v):
                getattr(d, k)[i] = x
        else:
            setattr(d, k, v)
    return d


EINVAL = {"cols 0": dict(cols=0), "cols 33": dict(cols=33), "rows 0": dict(rows=0), "rows 33": dict(rows=33),
          "tile_w 0": dict(tile_w=0), "tile_w 4097": dict(tile_w=4097), "tile_h 0": dict(tile_h=0), "tile_h 4097": dict(tile_h=4097),
          "W below the tile": dict(W=63), "W 4097": dict(W=4097), "H below the tile": dict(H=63), "H 4097": dict(H=4097),
          "overlap -1": dict(overlap=-1), "overlap = tile": dict(overlap=64),
          "xs[0] != 0": dict(xs=[1]), "xs not increasing": dict(xs=[0, 96, 96]), "xs step above tile - overlap": dict(xs=[0, 47, 96]),
          "xs does not end at W": dict(W=168), "ys[0] != 0": dict(ys=[2]), "ys step above tile - overlap": dict(ys=[0, 49], H=113),
          "ys does not end at H": dict(H=120), "a second zero": dict(xs=[0, 0, 96]),
          # a valid grid of 32 x 6 tiles of 2048 x 2048: 192 x 12 MiB
          "2^31 bytes": dict(W=4096, H=4096, tile_w=2048, tile_h=2048, cols=32, rows=6, overlap=0, xs=list(range(31)) + [2048],
                             ys=[0, 1, 2, 3, 4, 2048])}


@pytest.mark.parametrize("case", list(EINVAL), ids=list(EINVAL))
def test_einval_before_anything_is_enqueued(case):
    from sdlcm_amd import lib
    L = lib.load()
    tiles = torch.zeros(6, 64, 64, 3, dtype=torch.uint8, device=DEV)
    out = torch.full((113, 160, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    d = _desc(**EINVAL[case])
    rc = L.lcm_grid_combine_rgb8(C.c_void_p(tiles.data_ptr()), C.c_void_p(out.data_ptr()), C.byref(d), None)
    torch.cuda.synchronize()
    assert rc == -1, L.lcm_last_error()
    assert bool((out == SENTINEL).all())


def test_einval_for_null_pointers():
    from sdlcm_amd import lib
    L = lib.load()
    tiles = torch.zeros(6, 64, 64, 3, dtype=torch.uint8, device=DEV)
    out = torch.full((112, 160, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    t, o, d = C.c_void_p(tiles.data_ptr()), C.c_void_p(out.data_ptr()), _desc()
    assert L.lcm_grid_combine_rgb8(None, o, C.byref(d), None) == -1
    assert L.lcm_grid_combine_rgb8(t, None, C.byref(d), None) == -1
    assert L.lcm_grid_combine_rgb8(t, o, None, None) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert L.lcm_grid_combine_rgb8(t, o, C.byref(d), None) == 0           # the same call with everything in place runs
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the worker
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worker():
    os.environ["MODEL"] = "synthetic"
    os.environ.setdefault("MODEL_ROOT", "/nonexistent")
    from sdlcm_amd.backends.worker_factory import create_hip_worker
    w = create_hip_worker(worker_id=0)
    yield w
    w.close()


def _req(**kw):
    d = dict(prompt="a lighthouse at dusk", size="64x64", num_inference_steps=2, guidance_scale=1.0, seed=500, style_lora=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _job(req):
    return types.SimpleNamespace(req=req)


PIC_L, PIC_N = _pic(56, 80, 5), _pic(88, 104, 6)                      # 80 x 56 for Lanczos x 2; 104 x 88 for "None"
LANCZOS = dict(init_image=PIC_L, denoising_strength=0.5, script_name="SD upscale", script_args=[None, 16, "Lanczos", 2])
NONE = dict(init_image=PIC_N, denoising_strength=0.5, script_name="SD upscale", script_args=[None, 40, "None"])
_REFS = {}


def _reference(worker, which, **extra):
    """A1111's paste of the PNGs the worker returns for the six tiles as ordinary image-to-image requests: their pictures the
    crops of the PIL-Lanczos-upscaled picture (of the picture itself for "None"), their seeds seed + k.  Once per case."""
    tag = (which, tuple(sorted(extra.items())))
    if tag not in _REFS:
        from PIL import Image
        fields = LANCZOS if which == "lanczos" else NONE
        W, H, ov = (160, 112, 16) if which == "lanczos" else (104, 88, 40)
        up = fields["init_image"]
        if which == "lanczos":
            up = np.asarray(Image.fromarray(up).resize((W, H), Image.LANCZOS))
        xs, ys = sr.geometry(W, H, 64, 64, ov)
        tiles = []
        for k, (x, y) in enumerate((x, y) for y in ys for x in xs):
            crop = np.ascontiguousarray(up[y:y + 64, x:x + 64])
            png, seed = worker.run_job(_job(_req(init_image=crop, denoising_strength=0.5, seed=500 + k, **extra)))
            assert seed == 500 + k
            tiles.append(_decode(png))
        assert len(tiles) == 6
        _REFS[tag] = sr.combine_pil(np.stack(tiles), W, H, ov, xs, ys)
    return _REFS[tag]


def test_lanczos_request_equals_the_paste_of_its_tiles(worker):
    eng = worker._engine
    want = _reference(worker, "lanczos")
    n0 = dict(eng.stats)
    png, seed = worker.run_job(_job(_req(**LANCZOS)))
    got = _decode(png)
    assert seed == 500 and got.shape == (112, 160, 3)            # today's code returns a 64 x 64 picture
    assert np.array_equal(got, want), int((got != want).sum())
    assert eng.stats["sdupscale_requests"] == n0["sdupscale_requests"] + 1 and eng.stats["sdupscale_tiles"] == n0["sdupscale_tiles"] + 6
    assert eng.stats["unet_evals"] == n0["unet_evals"] + 6 * 2 and eng.stats["img2img_requests"] == n0["img2img_requests"]
    # run_job_with_latents: the 8 x 8 pool of tile 0's final latents
    from PIL import Image
    crop0 = np.ascontiguousarray(np.asarray(Image.fromarray(PIC_L).resize((160, 112), Image.LANCZOS))[:64, :64])
    _, _, blob0 = worker.run_job_with_latents(_job(_req(init_image=crop0, denoising_strength=0.5, seed=500)))
    png2, seed2, blob = worker.run_job_with_latents(_job(_req(**LANCZOS)))
    assert png2 == png and seed2 == 500 and blob == blob0 and len(blob) == 512


def test_none_upscaler_three_deep_cover(worker):
    want = _reference(worker, "none")
    got = _decode(worker.run_job(_job(_req(**NONE)))[0])
    assert got.shape == (88, 104, 3) and np.array_equal(got, want), int((got != want).sum())


def test_same_bytes_whatever_the_passes_and_the_resampler(worker, monkeypatch):
    pipe = worker._engine.pipe
    base = worker.run_job(_job(_req(**LANCZOS)))[0]
    calls = []
    real = pipe.generate_img2img
    monkeypatch.setattr(pipe, "generate_img2img", lambda pe, seeds, *a, **kw: calls.append(len(seeds)) or real(pe, seeds, *a, **kw))
    assert worker.run_job(_job(_req(**LANCZOS)))[0] == base and calls == [4, 2]          # run twice; passes of 4 + 2
    plain = worker.run_job(_job(_req()))
    assert worker.run_job(_job(_req(**LANCZOS)))[0] == base                               # after a plain request in between
    for cap, passes in ((1, [1] * 6), (2, [2, 2, 2])):
        del calls[:]
        with monkeypatch.context() as m:
            m.setattr(type(pipe), "img2img_batch_cap", lambda self, *a, cap=cap, **kw: cap)
            assert worker.run_job(_job(_req(**LANCZOS)))[0] == base, cap
        assert calls == passes
    with monkeypatch.context() as m:
        m.setenv("LCM_RESIZE", "pil")
        assert worker.run_job(_job(_req(**LANCZOS)))[0] == base
        assert worker.run_job(_job(_req(**NONE)))[0] == worker.run_job(_job(_req(**NONE)))[0]
    none_hip = worker.run_job(_job(_req(**NONE)))[0]
    with monkeypatch.context() as m:
        m.setenv("LCM_RESIZE", "pil")
        assert worker.run_job(_job(_req(**NONE)))[0] == none_hip
    assert worker.run_job(_job(_req())) == plain


def test_other_requests_keep_their_bytes(worker):
    plain_req = _req(script_args=[None, 999, "ESRGAN"])          # without script_name the arguments are not read
    i2i_req = _req(init_image=_pic(64, 64, 9), denoising_strength=0.5, script_name="")
    plain, i2i = worker.run_job(_job(plain_req)), worker.run_job(_job(i2i_req))
    assert plain == worker.run_job(_job(_req())) and _decode(plain[0]).shape == (64, 64, 3)
    worker.run_job(_job(_req(**LANCZOS)))
    assert worker.run_job(_job(plain_req)) == plain and worker.run_job(_job(i2i_req)) == i2i


def test_an_ordinary_batch_of_fitted_uploads_keeps_its_bytes(worker, monkeypatch):
    """``_fit_pending`` uploads a source once for neighbouring slots that hold the same pixels object: requests that share an
    upload object, next to uploads of other sizes and one that needs no fit, get the bytes they get alone and under LCM_RESIZE=pil."""
    from sdlcm_amd.backends import fit
    eng = worker._engine
    shared, other = _pic(96, 80, 21), _pic(50, 50, 22)
    reqs = [_req(init_image=shared, denoising_strength=0.5, seed=1), _req(init_image=shared, denoising_strength=0.5, seed=2, resize_mode=1),
            _req(init_image=other, denoising_strength=0.5, seed=3), _req(init_image=_pic(64, 64, 23), denoising_strength=0.5, seed=4)]
    key = worker._job_key(reqs[0])
    assert all(worker._job_key(r) == key for r in reqs)
    items = [worker._prepare(r, key) for r in reqs]
    assert fit.is_pending(items[0][3]) and items[0][3].pixels is items[1][3].pixels and not fit.is_pending(items[3][3])
    got = eng.run_batch(key, items, 0)
    monkeypatch.setenv("LCM_RESIZE", "pil")
    for r, (rgb, _) in zip(reqs, got):
        item = worker._prepare(r, key)
        assert not fit.is_pending(item[3])
        assert np.array_equal(eng.run_batch(key, [item], 0)[0][0], rgb), r.seed


def _outcome(f):
    try:
        return f.result(600)
    except Exception as e:      # noqa
        return e


def test_drained_batches(worker):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import minipool
    second = dict(LANCZOS, init_image=_pic(56, 80, 7), seed=900)
    reqs = {0: _req(**LANCZOS), 1: _req(**dict(LANCZOS, script_args=[None, 16, "ESRGAN_4x"])), 2: _req(**second),
            3: _req(**dict(LANCZOS, init_image=_pic(512, 512, 8))), 4: _req(init_image=_pic(64, 64, 9), denoising_strength=0.5),
            5: _req(**dict(LANCZOS, script_args=[None, 64]))}
    bad = {1: "upscaler 'ESRGAN_4x' is not served", 3: "LCM_SDUPSCALE_MAX_TILES", 5: "overlap 64"}
    assert worker._job_key(reqs[0]) == worker._job_key(reqs[2])
    solo = {s: worker.run_job(_job(r)) for s, r in reqs.items() if s not in bad}
    assert solo[0][0] != solo[2][0]
    pool = minipool.MiniPool(lambda worker_id: worker, {"m": "synthetic"}, "m")
    worker.bind_queue(pool.q)
    gate, inside = threading.Event(), threading.Event()
    hold = pool.submit_job(minipool.CustomJob(handler=lambda: (inside.set(), gate.wait(30))))
    assert inside.wait(30)
    try:
        futs = [pool.submit_job(minipool.GenerationJob(req=reqs[s])) for s in sorted(reqs)]
        gate.set()
        hold.result(60)
        res = [_outcome(f) for f in futs]
        pool.q.join()
        for s in sorted(reqs):
            if s in bad:
                assert isinstance(res[s], RuntimeError) and bad[s] in str(res[s]), (s, res[s])
            else:
                assert res[s] == solo[s], s
    finally:
        worker.bind_queue(None)
        pool._worker = None
        pool.shutdown()


def test_the_sdxl_worker_refuses_the_request():
    from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker
    with pytest.raises(RuntimeError, match="SD upscale is not served by the SDXL worker"):
        HipLcmSDXLWorker._job_key(_req(**LANCZOS))


def test_run_jobs_names_what_it_does_not_serve(worker):
    with pytest.raises(RuntimeError, match="run_jobs does not serve requests with an upload"):
        worker.run_jobs([_job(_req(**LANCZOS))])


def test_a_sampler_steps_the_tiles(worker):
    eng = worker._engine
    want = _reference(worker, "lanczos", sampler_name="Euler")
    n0 = eng.stats["sampler_requests"]
    got = _decode(worker.run_job(_job(_req(sampler_name="Euler", **LANCZOS)))[0])
    assert got.shape == (112, 160, 3) and np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(want, _reference(worker, "lanczos")) and eng.stats["sampler_requests"] == n0 + 1
