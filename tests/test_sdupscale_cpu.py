"""SD upscale without a GPU: the integer definition of the combine against PIL's paste in A1111's order, the tile geometry's
facts, parsing and every error (backends/sdupscale.py), the memo, the batch keys and the tiles' seeds."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdlcm_amd  # noqa: E402,F401
import sdupscale_reference as sr  # noqa: E402
from sdlcm_amd.backends import fit as ft  # noqa: E402
from sdlcm_amd.backends import sdupscale as su  # noqa: E402
from sdlcm_amd.backends.hip_worker import HipLcmSDXLWorker, HipLcmWorker  # noqa: E402

PIC = np.zeros((56, 80, 3), np.uint8)      # 80 wide, 56 high


def _req(**kw):
    d = dict(prompt="a cat", size="64x64", num_inference_steps=2, guidance_scale=1.0, seed=7, style_lora=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _sdu(**kw):
    d = dict(init_image=PIC, denoising_strength=0.5, script_name="SD upscale", script_args=[None, 16, "Lanczos", 2])
    d.update(kw)
    return _req(**d)


@pytest.mark.parametrize("geo", sr.GEOMETRIES, ids=["x".join(map(str, g)) for g in sr.GEOMETRIES])
def test_integer_definition_equals_pil_paste(geo):
    W, H, tw, th, ov = geo
    xs, ys = sr.geometry(*geo)
    for tiles in (sr.random_tiles(*geo, seed=W + H), np.full((len(xs) * len(ys), th, tw, 3), 255, np.uint8)):
        a, p = sr.combine_int(tiles, W, H, ov, xs, ys), sr.combine_pil(tiles, W, H, ov, xs, ys)
        assert a.shape == (H, W, 3) and np.array_equal(a, p)


def test_geometry_facts_over_a_sweep():
    assert sr.axis(104, 64, 40) == [0, 20, 40]                   # three-deep cover
    assert sr.axis(1024, 512, 64) == [0, 256, 512] and sr.axis(64, 64, 16) == [0] and sr.axis(65, 64, 16) == [0, 1]
    assert sr.axis(77, 16, 7)[-1] == 61                          # 7 * (61 / 7) is 60.999... in floats: the last offset is set outright
    n = 0
    for tile in (8, 16, 48, 64, 96, 512):
        for ov in sorted({0, 1, 7, 8, tile // 4, tile // 2, tile - 8, tile - 1}):
            if not 0 <= ov < tile:
                continue
            for size in list(range(tile, tile + 70)) + [2 * tile, 3 * tile - ov, 8 * tile, 4096]:
                if size > 4096:
                    continue
                v = sr.axis(size, tile, ov)
                assert sr.facts(v, size, tile, ov), (size, tile, ov, v)
                assert tuple(v) == su.axis(size, tile, ov) and su.check_axis(v, size, tile, ov)
                n += 1
    assert n > 2000


def test_parsing_defaults_and_forms():
    assert su.parse_args(_req(), 512, 512) == (64, "Lanczos", 2.0)
    assert su.parse_args(_req(script_args=[]), 512, 512) == (64, "Lanczos", 2.0)
    assert su.parse_args(_req(script_args=[None]), 512, 512) == (64, "Lanczos", 2.0)
    assert su.parse_args(_req(script_args=["x", 32]), 512, 512) == (32, "Lanczos", 2.0)
    assert su.parse_args(_req(script_args=(None, 0, "lanczos")), 512, 512) == (0, "Lanczos", 2.0)
    assert su.parse_args(_req(script_args=[None, 8.0, 1, 1.5]), 64, 64) == (8, "Lanczos", 1.5)
    assert su.parse_args(_req(script_args=[None, 8, " LANCZOS ", 8]), 64, 64) == (8, "Lanczos", 8.0)
    for none in ("None", "none", 0):
        assert su.parse_args(_req(script_args=[None, 8, none, "not read"]), 64, 64) == (8, "None", None)
    for name in ("SD upscale", "sd upscale", "  SD Upscale "):
        assert su.active(_req(script_name=name))
    for name in (None, ""):
        assert not su.active(_req(script_name=name))
    overlap, upscaler, W, H, g = su.parse_sdupscale(_sdu(), (0.5, PIC), 64, 64)
    assert (overlap, upscaler, W, H) == (16, "Lanczos", 160, 112)
    assert g.xs == (0, 48, 96) and g.ys == (0, 48) and (g.cols, g.rows) == (3, 2) and g.tiles[4] == (48, 48)
    # int(src * scale) cut to a multiple of 8; "None" keeps the picture's size
    assert su.target_size(80, 56, "Lanczos", 1.3) == (104, 72) and su.target_size(81, 57, "None", None) == (81, 57)
    assert su.parse_sdupscale(_sdu(script_args=[None, 40, "None"], init_image=np.zeros((88, 104, 3), np.uint8)),
                              (0.5, np.zeros((88, 104, 3), np.uint8)), 64, 64)[2:4] == (104, 88)


ERRORS = [
    (dict(script_name="Ultimate SD upscale"), r"script_name 'Ultimate SD upscale' is not served: SD upscale is the script served"),
    (dict(script_name=5), r"SD upscale is the script served"),
    (dict(script_args="16"), r"Invalid script_args"),
    (dict(script_args=[None, 1, 2, 3, 4]), r"at most 4"),
    (dict(script_args=[None, -1]), r"overlap -1"), (dict(script_args=[None, 257]), r"overlap 257"),
    (dict(script_args=[None, 1.5]), r"overlap 1\.5"), (dict(script_args=[None, "16"]), r"overlap '16'"),
    (dict(script_args=[None, True]), r"overlap True"),
    (dict(script_args=[None, 64]), r"overlap 64: it must be below the tile's sides"),
    (dict(script_args=[None, 16, "ESRGAN_4x"]), r"upscaler 'ESRGAN_4x' is not served: this worker serves 'Lanczos' \(1\) and 'None' \(0\)"),
    (dict(script_args=[None, 16, "Nearest"]), r"'Lanczos' \(1\) and 'None' \(0\)"), (dict(script_args=[None, 16, 2]), r"upscaler 2"),
    (dict(script_args=[None, 16, None]), r"upscaler None"),
    (dict(script_args=[None, 16, "Lanczos", 0.5]), r"scale_factor 0\.5"), (dict(script_args=[None, 16, 1, 8.5]), r"scale_factor 8\.5"),
    (dict(script_args=[None, 16, 1, "2"]), r"scale_factor '2'"), (dict(script_args=[None, 16, 1, float("nan")]), r"scale_factor nan"),
    (dict(init_image=None), r"needs a picture"),
    (dict(init_image=np.zeros((24, 80, 3), np.uint8)), r"160x48, smaller than the 64x64 tile"),               # H < tile_h
    (dict(init_image=np.zeros((80, 60, 3), np.uint8), script_args=[None, 16, "None"]), r"60x80, smaller"),      # W < tile_w
    (dict(init_image=np.zeros((600, 80, 3), np.uint8), script_args=[None, 16, 1, 8]), r"640x4800, sides above 4096"),
    (dict(init_image=np.zeros((64, 2100, 3), np.uint8)), r"4200x128, sides above 4096"),
    (dict(init_image=np.zeros((512, 512, 3), np.uint8)), r"441 tiles .* more than LCM_SDUPSCALE_MAX_TILES=64"),
    (dict(init_image=np.zeros((64, 1100, 3), np.uint8), script_args=[None, 0, "None"], size="32x64"), r"more than 32 tile columns or rows"),
    (dict(init_image=np.zeros((1100, 64, 3), np.uint8), script_args=[None, 0, "None"], size="64x32"), r"more than 32 tile columns or rows"),
    (dict(mask=np.zeros((56, 80), np.uint8)), r"not combined"), (dict(enable_hr=True), r"not combined"),
    (dict(denoise_strength=0.5), r"not combined"), (dict(pass_number=2), r"not combined"),
    (dict(controlnet_image=np.zeros((64, 64, 3), np.uint8)), r"not combined"),
    (dict(subseed=3, subseed_strength=0.5), r"not combined"), (dict(seed_resize_from_w=128, seed_resize_from_h=128), r"not combined"),
    (dict(denoising_strength=0.01), r"denoising_strength"), (dict(init_image=b"\x89PNG not a picture"), r"init_image"),
    (dict(init_images=[PIC, PIC], init_image=None), r"init_images"), (dict(resize_mode=3), r"resize_mode 3"),
    (dict(size="64by64"), r"Invalid size"),
]


@pytest.mark.parametrize("fields,msg", ERRORS, ids=[str(i) for i in range(len(ERRORS))])
def test_every_error_names_its_field(fields, msg):
    with pytest.raises(RuntimeError, match=msg):
        HipLcmWorker._job_key(_sdu(**fields))


def test_the_tile_limit_follows_the_environment(monkeypatch):
    big = dict(init_image=np.zeros((160, 160, 3), np.uint8))            # 320 x 320: 7 x 7 tiles
    assert HipLcmWorker._job_key(_sdu(**big))[-2:] == (320, 320)
    monkeypatch.setenv("LCM_SDUPSCALE_MAX_TILES", "48")
    with pytest.raises(RuntimeError, match="49 tiles .*LCM_SDUPSCALE_MAX_TILES=48"):
        HipLcmWorker._job_key(_sdu(**big))


def test_the_sdxl_worker_refuses_the_script():
    with pytest.raises(RuntimeError, match="SD upscale is not served by the SDXL worker"):
        HipLcmSDXLWorker._job_key(_sdu())
    with pytest.raises(RuntimeError, match="SDXL"):
        HipLcmSDXLWorker._job_key(_req(script_name="sd upscale"))


def test_the_parse_is_remembered_on_the_request():
    req = _sdu()
    i2i = (0.5, PIC)
    a = su.parse_sdupscale(req, i2i, 64, 64)
    assert su.parse_sdupscale(req, i2i, 64, 64) is a and getattr(req, su._MEMO)[4] is a
    req.script_args = [None, 8, "Lanczos", 2]                    # another object: parsed again
    b = su.parse_sdupscale(req, i2i, 64, 64)
    assert b is not a and b[0] == 8
    assert su.parse_sdupscale(req, i2i, 64, 48) is not b            # another tile
    k1 = HipLcmWorker._job_key(req)
    assert HipLcmWorker._job_key(req) == k1


def test_a_request_without_the_script_has_todays_key():
    today = (64, 64, 2, 1.0, None, 0)
    for fields in (dict(), dict(script_name=None), dict(script_name=""), dict(script_args=[None, 999, "ESRGAN", -3]),
                   dict(script_name="", script_args="nonsense"), dict(script_name=None, script_args=[None, 16, "Lanczos", 2])):
        assert HipLcmWorker._job_key(_req(**fields)) == today
        assert HipLcmSDXLWorker._job_key(_req(**fields)) == today
        i2i = dict(init_image=PIC, denoising_strength=0.5)
        assert HipLcmWorker._job_key(_req(**fields, **i2i)) == today + ("img2img", 0.5)
        assert su.parse_sdupscale(_req(**fields, **i2i), (0.5, PIC), 64, 64) is None


def test_the_keys_shape():
    i2i_key = HipLcmWorker._job_key(_req(init_image=PIC, denoising_strength=0.5))
    key = HipLcmWorker._job_key(_sdu())
    assert key == i2i_key + ("sdupscale", 16, "Lanczos", 160, 112)
    assert su.split_key(key) == (i2i_key, (16, "Lanczos", 160, 112)) and su.split_key(i2i_key) == (i2i_key, None)
    # W x H come from the parse: another picture, another key; the index form and the case of a name change nothing
    assert HipLcmWorker._job_key(_sdu(init_image=np.zeros((64, 80, 3), np.uint8)))[-2:] == (160, 128)
    assert HipLcmWorker._job_key(_sdu(script_args=[None, 16, 1, 2.0], script_name=" sd upscale ")) == key
    assert HipLcmWorker._job_key(_sdu(script_args=[None, 40, "none"], init_image=np.zeros((88, 104, 3), np.uint8)))[-5:] == \
        ("sdupscale", 40, "None", 104, 88)
    # a sampler's ending stays with the image-to-image key; the chunk count of a long prompt stays last
    smp = HipLcmWorker._job_key(_sdu(sampler_name="Euler"))
    assert smp == i2i_key + ("sampler", "Euler", "normal") + key[-5:]
    long = HipLcmWorker._job_key(_sdu(prompt="a cat, " * 40))
    assert long[-2] == "ctx" and long[:-2] == key


def test_tiles_are_windows_of_one_grid_with_seeds_of_their_own(monkeypatch):
    assert su.tile_seeds(7, 6) == [7, 8, 9, 10, 11, 12]
    assert su.pass_sizes(6, 8, (1, 2, 4, 8)) == [4, 2] and su.pass_sizes(9, 8, (1, 2, 4, 8)) == [8, 1]
    assert su.pass_sizes(6, 2, (1, 2, 4, 8)) == [2, 2, 2] and su.pass_sizes(3, 1, (1, 2, 4, 8)) == [1, 1, 1]
    assert su.pass_sizes(7, 8, (1,)) == [1] * 7
    pic = np.random.default_rng(1).integers(0, 256, (56, 80, 3), dtype=np.uint8)
    g = su.grid(160, 112, 64, 64, 16)
    monkeypatch.setenv("LCM_RESIZE", "hip")
    pend, on_device = su.tile_pictures(pic, g)
    assert on_device and len(pend) == 6 and all(ft.is_pending(p) and p.pixels is pend[0].pixels for p in pend)
    assert [(p.fit_w, p.fit_h, p.x0, p.y0, p.width, p.height) for p in pend] == [(160, 112, x, y, 64, 64) for x, y in g.tiles]
    monkeypatch.setenv("LCM_RESIZE", "pil")
    host, on_device = su.tile_pictures(pic, g)
    from PIL import Image
    up = np.asarray(Image.fromarray(pic).resize((160, 112), Image.LANCZOS))
    assert not on_device and all(np.array_equal(t, up[y:y + 64, x:x + 64]) for t, (x, y) in zip(host, g.tiles))
