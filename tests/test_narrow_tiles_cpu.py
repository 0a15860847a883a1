"""The shipped narrow-tile table (narrow_plans_gfx950.json) is a table of its own beside the plan table: exact launch shapes of
the plan table that run a 32-column tile.  Host logic only."""
import json

from sdlcm_amd import autotune, lib


def test_shipped_narrow_table_is_well_formed():
    with open(lib.PACKAGED_NARROW) as f:
        raw = json.load(f)
    main = lib.read_plans(lib.PACKAGED_PLANS)
    tab = lib.read_narrow(lib.PACKAGED_NARROW)
    assert len(tab) == len(raw)
    for k, bn in raw.items():
        key = tuple(int(v) for v in k.split(","))
        assert len(key) == 5 and ",".join(str(v) for v in key) == k, k
        assert key in main, f"{k}: not a shape of the shipped plan table"
        assert key[0] in (0, 2) and key[2] % 32 == 0 and bn == 32, (k, bn)


def test_plan_table_keeps_its_tiles(monkeypatch):
    monkeypatch.delenv("LCM_TUNE_CACHE", raising=False)
    monkeypatch.delenv("LCM_TUNED_PLANS", raising=False)
    assert lib.known_plans() == lib.read_plans(lib.PACKAGED_PLANS)
    for tab in (lib.known_plans(), autotune._load_cache()):
        assert tab and all(int(v[1]) in (64, 128, 160) for v in tab.values())
    assert lib.narrow_plans() == lib.read_narrow(lib.PACKAGED_NARROW)


def test_tuned_plans_off_ignores_the_narrow_table_too(monkeypatch):
    monkeypatch.delenv("LCM_TUNE_CACHE", raising=False)
    monkeypatch.setenv("LCM_TUNED_PLANS", "0")
    assert lib.narrow_plans() == {}
    assert lib.known_plans() == {}


def test_first_use_candidate_rule():
    """The tuner offers the 32-column tile only on launches the library honours an entry on, and only where the 64-wide grid
    times the parts leaves CUs empty (<= 256 workgroups)."""
    gemm = dict(halo=False, geglu=False, m_img=256, splittable=False)
    assert autotune._narrow_candidate((0, 256, 1280, 1280, 1), gemm)                          # 4 x 20 workgroups x 1-2 parts
    assert not autotune._narrow_candidate((0, 4096, 320, 320, 1), dict(gemm, m_img=4096))     # 64 x 5 workgroups
    assert not autotune._narrow_candidate((0, 256, 1280, 1280, 8), gemm)                      # batched in z
    assert not autotune._narrow_candidate((0, 256, 1280, 1280, 1), dict(gemm, geglu=True))
    conv = dict(halo=True, W=8, m_img=64, splittable=True)
    assert not autotune._narrow_candidate((2, 64, 1280, 11520, 17), conv)                     # GroupNorm-fused form
    assert not autotune._narrow_candidate((2, 64, 1280, 5120, 16), dict(conv, phases=4))
