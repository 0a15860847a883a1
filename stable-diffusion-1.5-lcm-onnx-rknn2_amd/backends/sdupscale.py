"""SD upscale: the script an A1111 client selects with ``script_name: "SD upscale"`` and ``script_args`` on
``/sdapi/v1/img2img`` to turn a picture into a larger one -- the picture is upscaled (Lanczos), cut into overlapping tiles of the
request's ``size``, every tile goes through image-to-image, and the tiles are blended back together.  Read with ``getattr`` like
the other kinds.  No GPU code here: the tiles are ``fit.Pending`` windows of ONE resample grid (the upscaled picture never
exists), their passes are ``LcmHipPipeline.generate_img2img`` and the way back is one launch of ``lcm_grid_combine_rgb8``
(include/lcm_hip.h defines its bytes; DESIGN.md section 6 has the request's sequence).

The tile grid is written after A1111's ``images.split_grid`` as recalled, the blend after its ``combine_grid``; equality with
A1111 is unverified.  Stated deviations: when ``int(src * scale)`` is no multiple of 8 A1111 resamples twice (to the scaled size,
then to the multiple of 8), here the picture is resampled once to the multiple of 8; ``overlap`` 0 has no blend region (A1111
divides by zero).
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple, Tuple

import numpy as np

from . import fit as _fit

KEY_TAG = "sdupscale"             # batch keys of SD-upscale jobs end in (KEY_TAG, overlap, upscaler, W, H), ahead of any ("ctx", n)
SCRIPT = "sd upscale"
LANCZOS, NONE = "Lanczos", "None"
UPSCALERS = (NONE, LANCZOS)       # A1111 lists "None" first: script_args may carry the index instead of the name
DEFAULT_OVERLAP, MAX_OVERLAP = 64, 256
DEFAULT_SCALE, MIN_SCALE, MAX_SCALE = 2.0, 1.0, 8.0
MAX_SIDE = 4096                   # the combine launch's and the resampler's output domain (include/lcm_hip.h)
MAX_AXIS = 32                     # LCM_GRID_MAX_AXIS
DEFAULT_MAX_TILES = 64
NOT_COMBINED = "SD upscale is not combined with "
SDXL_ERROR = "script_name: SD upscale is not served by the SDXL worker (SD1.5 and SD 2.x only)"
_MEMO = "_lcm_sdupscale_parsed"


class Grid(NamedTuple):
    """The tile grid of a W x H picture: tile k = r * cols + c lies at (xs[c], ys[r])."""
    W: int
    H: int
    tile_w: int
    tile_h: int
    overlap: int
    xs: Tuple[int, ...]
    ys: Tuple[int, ...]

    @property
    def cols(self):
        return len(self.xs)

    @property
    def rows(self):
        return len(self.ys)

    @property
    def tiles(self):
        """[(x, y)] of the tiles in row-major order."""
        return [(x, y) for y in self.ys for x in self.xs]


def max_tiles() -> int:
    return max(1, int(os.environ.get("LCM_SDUPSCALE_MAX_TILES", "") or DEFAULT_MAX_TILES))


def is_sdupscale_key(key) -> bool:
    return len(key) >= 5 and key[-5] == KEY_TAG


def split_key(key):
    """A batch key without its ("ctx", n) ending -> (the key without its SD-upscale ending, None | (overlap, upscaler, W, H))."""
    if is_sdupscale_key(key):
        return tuple(key[:-5]), tuple(key[-4:])
    return key, None


def tail(sdu) -> tuple:
    return () if sdu is None else (KEY_TAG,) + tuple(sdu[:4])


def active(req) -> bool:
    """Does the request select the script?  Absent, None or "" is today's request; any other name than the one served is the
    job's error."""
    name = getattr(req, "script_name", None)
    if name is None or (isinstance(name, str) and name == ""):
        return False
    if isinstance(name, str) and name.strip().lower() == SCRIPT:
        return True
    raise RuntimeError(f"script_name {name!r} is not served: SD upscale is the script served")


def axis(size: int, tile: int, overlap: int) -> Tuple[int, ...]:
    """The tile offsets of one axis, in Python floats (after images.split_grid).  Facts (checked by ``check_axis``; the combine
    launch relies on them): the first is 0 and no other is; they rise strictly, by at most tile - overlap; the last ends at size.
    The last offset is size - tile outright: (n - 1) * d can round to just below it in floats (size 77, tile 16, overlap 7 gives
    60.999...), which would leave the picture's last column under no tile."""
    n = math.ceil((size - overlap) / (tile - overlap))
    d = (size - tile) / (n - 1) if n > 1 else 0
    out = []
    for k in range(n):
        v = int(k * d)
        if v + tile >= size or k == n - 1:
            v = size - tile
        out.append(v)
    return tuple(out)


def check_axis(v, size: int, tile: int, overlap: int) -> bool:
    return (len(v) >= 1 and v[0] == 0 and v[-1] + tile == size
            and all(b > a and b - a <= tile - overlap for a, b in zip(v, v[1:])))


def grid(W: int, H: int, tile_w: int, tile_h: int, overlap: int) -> Grid:
    return Grid(int(W), int(H), int(tile_w), int(tile_h), int(overlap), axis(W, tile_w, overlap), axis(H, tile_h, overlap))


def _integer(v, what, lo, hi):
    try:
        if isinstance(v, (bool, str, bytes)) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError
        return int(v)
    except (TypeError, ValueError, OverflowError):
        raise RuntimeError(f"Invalid script_args {what} {v!r}, expected an integer in {lo}..{hi}")


def _upscaler(v):
    if isinstance(v, str):
        for name in UPSCALERS:
            if v.strip().lower() == name.lower():
                return name
    elif not isinstance(v, (bool, bytes)):
        try:
            if int(v) == v and 0 <= int(v) < len(UPSCALERS):
                return UPSCALERS[int(v)]
        except (TypeError, ValueError, OverflowError):
            pass
    raise RuntimeError(f"script_args upscaler {v!r} is not served: this worker serves 'Lanczos' (1) and 'None' (0)")


def _scale(v):
    try:
        if isinstance(v, (bool, str, bytes)):
            raise ValueError
        f = float(v)
        if not (math.isfinite(f) and MIN_SCALE <= f <= MAX_SCALE):
            raise ValueError
        return f
    except (TypeError, ValueError, OverflowError):
        raise RuntimeError(f"Invalid script_args scale_factor {v!r}, expected a number in [{MIN_SCALE:g}, {MAX_SCALE:g}]")


def parse_args(req, tile_w: int, tile_h: int):
    """``script_args`` = [ignored, overlap, upscaler, scale_factor] (A1111's order; missing trailing entries take the defaults)
    -> (overlap, upscaler name, scale | None for "None")."""
    args = getattr(req, "script_args", None)
    if args is None:
        args = ()
    if not isinstance(args, (list, tuple)):
        raise RuntimeError(f"Invalid script_args: expected a list [ignored, overlap, upscaler, scale_factor], got {type(args).__name__}")
    if len(args) > 4:
        raise RuntimeError(f"Invalid script_args: expected at most 4 entries [ignored, overlap, upscaler, scale_factor], got {len(args)}")
    overlap = _integer(args[1], "overlap", 0, MAX_OVERLAP) if len(args) > 1 else DEFAULT_OVERLAP
    if overlap >= min(tile_w, tile_h):
        raise RuntimeError(f"Invalid script_args overlap {overlap}: it must be below the tile's sides ({tile_w}x{tile_h})")
    upscaler = _upscaler(args[2]) if len(args) > 2 else LANCZOS
    scale = None
    if upscaler == LANCZOS:
        scale = _scale(args[3]) if len(args) > 3 else DEFAULT_SCALE
    return overlap, upscaler, scale


def target_size(src_w: int, src_h: int, upscaler: str, scale):
    """The grid's size: the picture's own for "None"; for "Lanczos" int(side * scale) cut to a multiple of 8."""
    if upscaler == NONE:
        return int(src_w), int(src_h)
    return int(src_w * scale) // 8 * 8, int(src_h * scale) // 8 * 8


def parse_sdupscale(req, i2i, tile_w: int, tile_h: int):
    """-> None for a request that does not select the script (whatever its ``script_args`` says: today's key and bytes), else
    (overlap, upscaler, W, H, Grid).  i2i: ``img2img.parse_img2img(req)`` (the picture gives W x H).  RuntimeError for the job that
    carries the bad field.  The parse is remembered on the request object (the batch key is computed more than once per job)."""
    if not active(req):
        return None
    if i2i is None:
        raise RuntimeError("script_name 'SD upscale' needs a picture (init_image / init_images)")
    name, args, pic = getattr(req, "script_name", None), getattr(req, "script_args", None), i2i[1]
    memo = getattr(req, _MEMO, None)
    if memo is not None and memo[0] is name and memo[1] is args and memo[2] is pic and memo[3] == (tile_w, tile_h, max_tiles()):
        return memo[4]
    if tile_w < 1 or tile_h < 1:
        raise RuntimeError(f"Invalid size {tile_w}x{tile_h} for SD upscale tiles")
    overlap, upscaler, scale = parse_args(req, tile_w, tile_h)
    W, H = target_size(pic.shape[1], pic.shape[0], upscaler, scale)
    if W < tile_w or H < tile_h:
        raise RuntimeError(f"SD upscale: the {'upscaled ' if upscaler == LANCZOS else ''}picture is {W}x{H}, smaller than the "
                           f"{tile_w}x{tile_h} tile (size)")
    if W > MAX_SIDE or H > MAX_SIDE:
        raise RuntimeError(f"SD upscale: the upscaled picture would be {W}x{H}, sides above {MAX_SIDE} are not served")
    g = grid(W, H, tile_w, tile_h, overlap)
    if g.cols > MAX_AXIS or g.rows > MAX_AXIS:
        raise RuntimeError(f"SD upscale: {g.cols} x {g.rows} tiles, more than {MAX_AXIS} tile columns or rows are not served")
    if g.cols * g.rows > max_tiles():
        raise RuntimeError(f"SD upscale: {g.cols * g.rows} tiles of {tile_w}x{tile_h} for a {W}x{H} picture, more than "
                           f"LCM_SDUPSCALE_MAX_TILES={max_tiles()}")
    if not (check_axis(g.xs, W, tile_w, overlap) and check_axis(g.ys, H, tile_h, overlap)):
        raise RuntimeError(f"SD upscale: no valid tile grid for {W}x{H}, tile {tile_w}x{tile_h}, overlap {overlap}")
    out = (overlap, upscaler, W, H, g)
    try:
        object.__setattr__(req, _MEMO, (name, args, pic, (tile_w, tile_h, max_tiles()), out))
    except Exception:
        pass
    return out


def tile_seeds(seed: int, n: int):
    """Tile k is the image-to-image request of its own pixels with seed + k (A1111 with ``batch_size`` 1)."""
    return [int(seed) + k for k in range(n)]


def tile_pictures(pic: np.ndarray, g: Grid):
    """-> ([the T tiles' pictures for ``generate_img2img``, row-major], fitted on the device?).  On the device path
    (LCM_RESIZE=hip and inside ``fit.in_domain``) tile k is the ``fit.Pending`` window at (x_c, y_r) of the ONE W x H resample
    grid of the picture -- every one holds the same ``pixels`` object, so a pass uploads the source once -- and the upscaled
    picture never exists; a grid of the source's size takes the resampler's copy path.  Otherwise the host resamples once with PIL
    and the tiles are host crops.  Both give the same bytes."""
    sh, sw = pic.shape[:2]
    if _fit.backend() == "hip" and _fit.in_domain(sw, sh, 3, g.W, g.H) and _fit.in_domain(1, 1, 1, g.tile_w, g.tile_h):
        src = np.ascontiguousarray(pic)
        return [_fit.Pending(src, g.W, g.H, x, y, g.tile_w, g.tile_h) for x, y in g.tiles], True
    up = pic
    if (sw, sh) != (g.W, g.H):
        from PIL import Image
        up = np.asarray(Image.fromarray(pic, "RGB").resize((g.W, g.H), Image.LANCZOS), dtype=np.uint8)
    return [np.ascontiguousarray(up[y:y + g.tile_h, x:x + g.tile_w]) for x, y in g.tiles], False


def pass_sizes(n: int, cap: int, sizes):
    """The tiles' passes in row-major order: each the largest of ``sizes`` that fits both the remaining tiles and ``cap``."""
    sizes = sorted(set(int(s) for s in sizes) | {1})
    out = []
    while n > 0:
        m = max(s for s in sizes if s <= n and (s <= cap or s == 1))
        out.append(m)
        n -= m
    return out
