"""Host side of the ControlNet preprocessors: the numpy reference's own hand cases (tests/canny_reference.py), parsing of
``controlnet_module`` / ``controlnet_threshold_a`` / ``controlnet_threshold_b``, defaults, errors, the memo and the batch keys.
No GPU."""
from dataclasses import dataclass, field
from typing import Any, Optional

import numpy as np
import pytest

import canny_reference as cy
from sdlcm_amd import lib
from sdlcm_amd.backends import controlnet as cnb
from sdlcm_amd.backends.hip_worker import HipLcmWorker


@dataclass
class _Style:
    style: Optional[str] = None
    level: int = 0


@dataclass
class _Req:
    prompt: str = "p"
    size: str = "64x64"
    num_inference_steps: int = 2
    guidance_scale: float = 1.0
    seed: Optional[int] = 1
    style_lora: _Style = field(default_factory=_Style)
    controlnet_image: Any = None
    controlnet_conditioning_scale: Optional[float] = None
    controlnet_module: Any = None
    controlnet_threshold_a: Any = None
    controlnet_threshold_b: Any = None


@dataclass
class _OldReq:
    """A request of a client that knows nothing of modules: the fields do not exist."""
    prompt: str = "p"
    size: str = "64x64"
    num_inference_steps: int = 2
    guidance_scale: float = 1.0
    seed: Optional[int] = 1
    style_lora: _Style = field(default_factory=_Style)
    controlnet_image: Any = None


def _photo(seed=0):
    return cy.smoothed_noise(64, 64, seed)


def _step():
    img = np.zeros((8, 8, 3), np.uint8)
    img[:, 4:] = 255
    return img


# ---- the reference's hand cases ------------------------------------------------------------------------------------------------
def test_reference_step_edge_is_column_3():
    e = cy.canny(_step(), 100, 200)
    want = np.zeros((8, 8), bool)
    want[:, 3] = True
    assert e.dtype == np.uint8 and e.shape == (8, 8, 3)
    assert np.array_equal(e[..., 0] == 255, want) and np.array_equal(e[..., 0], e[..., 1]) and np.array_equal(e[..., 0], e[..., 2])
    assert set(np.unique(e)) == {0, 255} and int((e[..., 0] == 255).sum()) == 8
    t = cy.canny(np.ascontiguousarray(_step().transpose(1, 0, 2)), 100, 200)
    assert np.array_equal(t[..., 0] == 255, want.T)


def test_reference_step_magnitude_is_1020():
    dx, dy, m = cy.gradients(_step())
    assert np.all(m[:, 3] == 1020) and np.all(m[:, 4] == 1020) and np.all(dx[:, 3] == 1020) and np.all(dy == 0)
    assert np.all(cy.classes(_step(), 100, 1019)[:, 3] == 2)
    assert np.all(cy.classes(_step(), 100, 1020)[:, 3] == 1)
    assert not cy.classes(_step(), 1020, 1020).any()
    assert not cy.canny(_step(), 100, 1020).any()           # weak only: nothing to link to
    assert not cy.canny(_step(), 1020, 1020).any()


def test_reference_small_and_flat_pictures():
    assert not cy.canny(np.full((1, 1, 3), 200, np.uint8)).any()
    assert not cy.canny(np.zeros((5, 7, 3), np.uint8)).any()
    assert cy.thresholds(200.9, 100.2) == (100, 200) and cy.thresholds(1, 1) == (1, 1)
    a = cy.smoothed_noise(24, 40, 3)
    assert np.array_equal(cy.canny(a, 200, 100), cy.canny(a, 100, 200))
    assert np.array_equal(cy.canny(np.stack([a, a[::-1]]), 50, 90)[1], cy.canny(np.ascontiguousarray(a[::-1]), 50, 90))


def test_reference_channel_pick_and_tie_rules():
    img = np.zeros((6, 6, 3), np.uint8)
    img[:, 3:, 2] = 200                                      # only channel 2 has an edge
    dx, dy, m = cy.gradients(img)
    assert m[2, 2] == 800 and dx[2, 2] == 800
    gray = np.repeat(cy.smoothed_noise(16, 16, 1)[..., :1], 3, axis=2)
    g0 = cy.gradients(gray)
    one = gray.copy()
    one[..., 1:] = 0                                         # channel 0 alone gives the same pick as the three-way tie
    g1 = cy.gradients(one)
    inner = (slice(1, -1), slice(1, -1))
    assert all(np.array_equal(a[inner], b[inner]) for a, b in zip(g0, g1))
    # a two-pixel plateau of equal magnitudes: the left pixel loses (m > left holds for it, m >= right too; the right one fails
    # m > left), so exactly one column of the plateau survives
    cls = cy.classes(_step(), 100, 200)
    assert np.all(cls[:, 3] == 2) and not cls[:, 4].any()


def test_reference_link_and_spirals():
    for h, w, rounds in ((64, 64, 2047), (40, 72, 1439)):
        s = cy.spiral(h, w)
        assert int((s == 2).sum()) == 1 and cy.growth_rounds(s) == rounds
        assert np.array_equal(cy.link(s), s > 0)             # everything hangs on the one strong pixel
        assert not cy.link(cy.spiral(h, w, strong=False)).any()
    d = np.zeros((4, 4), np.uint8)
    d[0, 0], d[1, 1], d[3, 3] = 2, 1, 1                      # diagonal contact links, a gap does not
    want = np.zeros((4, 4), bool)
    want[0, 0] = want[1, 1] = True
    assert np.array_equal(cy.link(d), want)


# ---- parsing ---------------------------------------------------------------------------------------------------------------------
def test_no_module_is_todays_request():
    photo = _photo()
    for r in (_Req(controlnet_image=photo), _Req(controlnet_image=photo, controlnet_module="none"),
              _Req(controlnet_image=photo, controlnet_module="None"), _OldReq(controlnet_image=photo)):
        out = cnb.parse_control(r)
        assert out[0] == 1.0 and out[1] is not None and len(out) == 2 and np.array_equal(out[1], photo)
        assert cnb.parse_preprocessor(r) == ()
    for r in (_Req(), _OldReq(), _Req(controlnet_module="none", controlnet_threshold_a=7)):
        assert cnb.parse_control(r) is None and cnb.parse_preprocessor(r) is None


def test_module_defaults_and_thresholds():
    photo = _photo()
    mk = lambda **kw: _Req(controlnet_image=photo, **kw)
    assert cnb.parse_preprocessor(mk(controlnet_module="canny")) == ("canny", 100, 200)
    assert (cnb.CANNY_LOW, cnb.CANNY_HIGH) == (100, 200) and cnb.MODULES == ("none", "canny", "invert")
    assert cnb.parse_preprocessor(mk(controlnet_module="Canny", controlnet_threshold_a=20, controlnet_threshold_b=60.7)) == ("canny", 20, 60)
    assert cnb.parse_preprocessor(mk(controlnet_module="canny", controlnet_threshold_a=255, controlnet_threshold_b=1)) == ("canny", 1, 255)
    assert cnb.parse_preprocessor(mk(controlnet_module="canny", controlnet_threshold_b=50.5)) == ("canny", 50, 100)
    assert cnb.parse_preprocessor(mk(controlnet_module="invert", controlnet_threshold_a=-4)) == ("invert",)   # takes no parameters
    assert cnb.parse_control(mk(controlnet_module="canny", controlnet_conditioning_scale=0.5))[0] == 0.5


@pytest.mark.parametrize("fields,word", [
    (dict(controlnet_module="depth"), "controlnet_module"),
    (dict(controlnet_module="openpose_full"), "'none', 'canny', 'invert'"),
    (dict(controlnet_module=3), "controlnet_module"),
    (dict(controlnet_module="canny", controlnet_threshold_a=0), "controlnet_threshold_a"),
    (dict(controlnet_module="canny", controlnet_threshold_a=0.99), "controlnet_threshold_a"),
    (dict(controlnet_module="canny", controlnet_threshold_a=255.5), "controlnet_threshold_a"),
    (dict(controlnet_module="canny", controlnet_threshold_b=256), "controlnet_threshold_b"),
    (dict(controlnet_module="canny", controlnet_threshold_b=float("nan")), "controlnet_threshold_b"),
    (dict(controlnet_module="canny", controlnet_threshold_b="200"), "controlnet_threshold_b"),
    (dict(controlnet_module="canny", controlnet_threshold_a=True), "controlnet_threshold_a"),
    (dict(controlnet_module="canny", controlnet_threshold_a=[100]), "controlnet_threshold_a"),
])
def test_new_errors_with_an_image(fields, word):
    r = _Req(controlnet_image=_photo(), **fields)
    for call in (cnb.parse_control, cnb.parse_preprocessor, HipLcmWorker._job_key):
        with pytest.raises(RuntimeError, match=word):
            call(r)


def test_module_without_an_image_raises():
    for name in ("canny", "invert", " Canny "):
        with pytest.raises(RuntimeError, match="controlnet_image"):
            cnb.parse_control(_Req(controlnet_module=name))
        with pytest.raises(RuntimeError, match="controlnet_image"):
            HipLcmWorker._job_key(_Req(controlnet_module=name))


def test_existing_errors_are_unchanged():
    with pytest.raises(RuntimeError, match="Invalid controlnet_conditioning_scale 2.5, expected a number in \\[0.0, 2.0\\]"):
        cnb.parse_control(_Req(controlnet_image=_photo(), controlnet_conditioning_scale=2.5, controlnet_module="canny"))
    with pytest.raises(RuntimeError, match="Invalid controlnet_image: not a decodable PNG or JPEG"):
        cnb.parse_control(_Req(controlnet_image=b"junk", controlnet_module="canny"))
    with pytest.raises(RuntimeError, match="Invalid controlnet_image: expected an H x W x 3 uint8 array"):
        cnb.parse_control(_Req(controlnet_image=np.zeros((4, 4), np.uint8)))


def test_memo_follows_module_and_thresholds():
    photo = _photo()
    r = _Req(controlnet_image=photo)
    a = cnb.parse_control(r)
    assert cnb.parse_control(r)[1] is a[1]                   # remembered: the same decoded array
    assert cnb.parse_preprocessor(r) == ()
    r.controlnet_module = "canny"
    assert cnb.parse_preprocessor(r) == ("canny", 100, 200) and cnb.parse_control(r)[1] is a[1]
    r.controlnet_threshold_a = 30
    assert cnb.parse_preprocessor(r) == ("canny", 30, 200)
    r.controlnet_threshold_b = 20.0
    assert cnb.parse_preprocessor(r) == ("canny", 20, 30)
    r.controlnet_module = "invert"
    assert cnb.parse_preprocessor(r) == ("invert",)
    r.controlnet_conditioning_scale = 0.25
    assert cnb.parse_control(r)[0] == 0.25
    r.controlnet_module = "pose"
    with pytest.raises(RuntimeError, match="controlnet_module"):
        cnb.parse_preprocessor(r)
    r.controlnet_module = None
    assert cnb.parse_preprocessor(r) == ()
    other = _photo(5)
    r.controlnet_image = other
    assert np.array_equal(cnb.parse_control(r)[1], other)


# ---- batch keys ----------------------------------------------------------------------------------------------------------------
def test_keys():
    photo = _photo()
    plain = HipLcmWorker._job_key(_OldReq())
    assert len(plain) == 6 and plain == (64, 64, 2, 1.0, None, 0)
    hint = HipLcmWorker._job_key(_OldReq(controlnet_image=photo))
    assert hint == plain + ("controlnet", 1.0)
    # no module, or "none": today's keys, with and without a hint
    assert HipLcmWorker._job_key(_Req()) == plain and HipLcmWorker._job_key(_Req(controlnet_module="none")) == plain
    assert HipLcmWorker._job_key(_Req(controlnet_image=photo)) == hint
    assert HipLcmWorker._job_key(_Req(controlnet_image=photo, controlnet_module="none", controlnet_threshold_a=3)) == hint
    # stray fields of a plain request are not read
    assert HipLcmWorker._job_key(_Req(controlnet_threshold_a=100, controlnet_threshold_b=200)) == plain
    assert HipLcmWorker._job_key(_Req(controlnet_module="none", controlnet_threshold_a=-1, controlnet_threshold_b="x")) == plain
    assert HipLcmWorker._job_key(_Req(controlnet_module="depth_midas")) == plain
    # modules: the tail after the scale
    kc = HipLcmWorker._job_key(_Req(controlnet_image=photo, controlnet_module="canny"))
    assert kc == hint + ("canny", 100, 200)
    ks = HipLcmWorker._job_key(_Req(controlnet_image=photo, controlnet_module="canny", controlnet_conditioning_scale=0.5,
                                    controlnet_threshold_a=20, controlnet_threshold_b=60))
    assert ks == plain + ("controlnet", 0.5, "canny", 20, 60)
    ki = HipLcmWorker._job_key(_Req(controlnet_image=photo, controlnet_module="invert"))
    assert ki == hint + ("invert",)
    assert len({hint, kc, ks, ki}) == 4
    for k in (hint, kc, ks, ki):
        assert cnb.is_control_key(k) and k[7] in (1.0, 0.5)
    assert not cnb.is_control_key(plain)
    assert cnb.key_preprocessor(hint) == () and cnb.key_preprocessor(kc) == ("canny", 100, 200) and cnb.key_preprocessor(ki) == ("invert",)
    # swapped thresholds are the same pass
    assert HipLcmWorker._job_key(_Req(controlnet_image=photo, controlnet_module="canny", controlnet_threshold_a=200,
                                      controlnet_threshold_b=100)) == kc


def test_abi_lists_the_new_entry_points():
    for name in ("lcm_canny_ws_bytes", "lcm_canny_classes_u8", "lcm_canny_link", "lcm_canny_rgb8", "lcm_invert_u8"):
        assert name in lib.EXPORTS
