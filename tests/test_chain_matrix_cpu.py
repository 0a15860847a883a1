"""What entitles tests/chain_reference.py's ChainOracle to judge the cells of tests/test_chain_matrix_gpu.py, on the CPU.

1. Where a trusted chain oracle exists, the new one gives its final latents bit for bit (np.array_equal): RefineChainOracle,
   HiresChainOracle with and without negative embeddings, inpaint_reference.cpu_chain, and LCMPipelineOracle with the
   v-prediction scheduler at guidance 1 and 7.5.
2. Every wiring mutant that applies to a cell lies at least SEPARATION = 10 latent bounds and at least 10 x 1e-2 on the [0,1]
   image from the true oracle, at the very inputs the GPU test uses, for both requests of the cell's pair (neg_rows_rotated
   pairs a request with the other one's negative embeddings).  A GPU result within one bound of the true oracle is then at least 9 bounds from every mutant.

Measured separations, the smaller of the two requests (latents in bounds of 5e-3 max(1, g) std(oracle latents) | image [0,1]
max|d|); "-" = the mutant does not apply:
  cell               wrong_pred   noise_shift  renoise_next kept_current kept_at_end  cfg_swapped  cfg_dropped  neg_rotated  uncond_stale
  hires-b-64x64      14211|1.00   -            223|0.34     -            -            -            -            -            -
  hires-c-64x64      6500|1.00    -            108|0.31     -            -            219|0.54     77|0.19      81|0.29      146|0.56
  refine-a-64x64     200|1.00     18|0.12      255|0.21     -            -            71|0.49      28|0.20      36|0.19      30|0.20
  refine-b-64x64     13349|1.00   624|0.86     288|0.35     -            -            -            -            -            -
  refine-c-64x64     5925|1.00    257|0.94     131|0.38     -            -            218|0.57     80|0.20      106|0.32     137|0.45
  img2img-a-64x64    144|0.94     94|0.49      32|0.25      -            -            106|0.71     42|0.30      50|0.29      105|0.65
  img2img-b-64x64    1208|0.57    439|0.81     120|0.25     -            -            -            -            -            -
  img2img-c-64x64    538|0.71     252|0.88     62|0.30      -            -            162|0.56     58|0.18      62|0.22      84|0.39
  inpaint-a-64x64    189|1.00     122|0.60     47|0.33      39|0.23      39|0.23      137|0.62     51|0.31      61|0.30      141|0.72
  inpaint-b-64x64    1242|0.76    564|0.98     126|0.27     424|0.60     424|0.60     -            -            -            -
  inpaint-c-64x64    621|0.92     270|1.00     70|0.29      195|0.61     195|0.61     219|0.80     74|0.25      82|0.35      102|0.45
  variation-a-64x64  199|1.00     -            -            -            -            82|0.49      33|0.18      33|0.22      34|0.19
  variation-c-64x64  7315|1.00    -            -            -            -            154|0.48     50|0.15      59|0.29      187|0.57
  hires-c-64x96      6068|1.00    -            89|0.27      -            -            183|0.51     60|0.17      50|0.17      166|0.52
  refine-c-64x96     8138|1.00    243|0.78     140|0.38     -            -            184|0.43     59|0.15      59|0.13      129|0.41
  img2img-c-64x96    588|0.49     255|0.73     60|0.24      -            -            183|0.41     60|0.15      46|0.15      117|0.36
  inpaint-c-64x96    701|0.68     298|0.81     72|0.31      229|0.61     229|0.63     229|0.50     74|0.20      54|0.20      133|0.46
  variation-c-64x96  6936|1.00    -            -            -            -            145|0.37     49|0.16      53|0.15      196|0.53
"""
import numpy as np
import pytest
import torch

import chain_reference as cr
import hires_reference as hr
import inpaint_reference as ir
import refine_reference as rr


# ---- 1. the overlap with the trusted oracles ----------------------------------------------------------------------------------
def _embeds(D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 77, D, generator=g).half().float(), torch.randn(1, 77, D, generator=g).half().float()


@pytest.fixture(scope="module")
def sd15():
    from sdlcm_amd import weights
    return weights.synthetic_unet(), weights.synthetic_vae(), weights.synthetic_vae_encoder()


def _same(name, a, b):
    ok = np.array_equal(np.asarray(a), np.asarray(b))
    print(f"[chain-matrix] overlap {name}: final latents {'equal bit for bit' if ok else 'DIFFER, max|d| = %.3g' % np.abs(np.asarray(a) - np.asarray(b)).max()}")
    assert ok, name


def test_equals_the_refine_oracle(sd15):
    usd, vsd, _ = sd15
    pe, _ = _embeds(768, 1)
    ref = rr.RefineChainOracle(usd, vsd)(pe, 64, 64, 2, 1.5, 31, 0.6, 2)
    got = cr.ChainOracle(usd, vsd)(pe, 64, 64, 2, 1.5, 31, kind=cr.refine(0.6, 2), decode=False)
    for k in range(3):
        _same(f"RefineChainOracle x^{k}", got["xk"][k], ref["xk"][k])
    _same("RefineChainOracle", got["latents"], ref["xk"][-1])


def test_equals_the_hires_oracle_with_and_without_negative_embeds(sd15):
    from sdlcm_amd import weights
    from sdlcm_amd.config import unet_config
    usd, vsd, _ = sd15
    pe, ne = _embeds(768, 2)
    hires = (96, 96, 2, 0.7, hr.BICUBIC)
    ref = hr.HiresChainOracle(usd, vsd)(pe, 64, 64, 2, 1.0, 32, hires)
    got = cr.ChainOracle(usd, vsd)(pe, 64, 64, 2, 1.0, 32, kind=cr.hires(*hires), decode=False)
    _same("HiresChainOracle, embedded guidance (lowres)", got["lowres"], ref["lowres"])
    _same("HiresChainOracle, embedded guidance", got["latents"], ref["latents"])
    nocond = dict(time_cond_proj_dim=None)
    usd_n = weights.synthetic_unet(nocond)
    ref = hr.HiresChainOracle(usd_n, vsd, unet_config(nocond))(pe, 64, 64, 2, 3.0, 33, hires, negative_embeds=ne)
    got = cr.ChainOracle(usd_n, vsd, unet_config(nocond))(pe, 64, 64, 2, 3.0, 33, kind=cr.hires(*hires), negative_embeds=ne, decode=False)
    _same("HiresChainOracle, negative_embeds at g = 3", got["latents"], ref["latents"])


def test_equals_the_inpaint_cpu_chain(sd15):
    usd, vsd, esd = sd15
    pe, _ = _embeds(768, 3)
    pic = cr.picture(64, 64, 51)
    half = np.zeros((1, 64, 64), np.uint8)
    half[0, :, 28:] = 255
    M = ir.latent_mask(ir.blur(half, 4))[0]
    assert 0 < M.sum() < M.size
    ref = ir.cpu_chain(rr.RefineChainOracle(usd, vsd), esd, pe, pic, M, 2, 0.5, 34)
    got = cr.ChainOracle(usd, vsd, enc_sd=esd)(pe, 64, 64, 2, 1.0, 34, kind=cr.inpaint(pic, M, 0.5), decode=False)
    _same("inpaint_reference.cpu_chain (z)", got["z"], ref["z"])
    _same("inpaint_reference.cpu_chain", got["latents"], ref["latents"])


@pytest.mark.parametrize("guidance", [1.0, 7.5])
def test_equals_the_pipeline_oracle_with_the_v_scheduler(guidance):
    from oracle.pipeline import LCMPipelineOracle
    from test_sd2_gpu import _oracle_scheduler
    usd, _, cfg, sch = _form("c")
    from sdlcm_amd import weights
    vsd = weights.synthetic_vae()
    pe, ne = _embeds(1024, 4)
    ora = LCMPipelineOracle(usd, vsd, cfg)
    ora.sched = _oracle_scheduler()
    ref = ora(pe, 64, 64, 2, guidance, 35, negative_embeds=ne if guidance > 1 else None)
    got = cr.ChainOracle(usd, vsd, cfg, schedule=sch)(pe, 64, 64, 2, guidance, 35, negative_embeds=ne if guidance > 1 else None, decode=False)
    _same(f"LCMPipelineOracle, v-prediction, g = {guidance}", got["latents"], ref["latents"])


# ---- 2. the mutants -----------------------------------------------------------------------------------------------------------
_FORMS = {}


def _form(form):
    """The weights of a form, built once per UNet (forms (b) and (c) share theirs)."""
    key = cr.FORMS[form][0]
    if key not in _FORMS:
        _FORMS[key] = cr.form_weights(form)
    return _FORMS[key]


_ORACLES = {}


def _oracle(form):
    from sdlcm_amd import weights
    key = cr.FORMS[form][0]
    if key not in _ORACLES:
        usd, _, cfg, sch = _form(form)
        _ORACLES[key] = cr.ChainOracle(usd, weights.synthetic_vae(), cfg, enc_sd=weights.synthetic_vae_encoder(), schedule=sch)
    return _ORACLES[key]


ALL_MUTANTS = tuple(dict.fromkeys(m for ms in cr.MUTANTS.values() for m in ms)) + cr.CFG_MUTANTS


@pytest.mark.parametrize("cell", cr.CELLS, ids=cr.cell_id)
def test_every_mutant_is_ten_bounds_from_the_oracle(cell):
    kind, form, _ = cell
    ora = _oracle(form)
    ora.forget()
    inp = cr.cell_inputs(cell)
    g = inp["guidance"]
    M = ir.latent_mask(ir.blur(inp["masks"], cr.MASK_BLUR)) if kind == "inpaint" else None
    name = "plain" if kind == "variation" else kind
    bad = []
    for b in range(2):                                   # both requests of the pair: the GPU test judges both
        Mb = None if M is None else M[b]
        if Mb is not None:
            assert 0 < Mb.sum() < Mb.size
        true = cr.oracle_run(ora, cell, inp, b, Mb)
        bound = cr.latent_bound(g, true["latents"])
        row = []
        for m in ALL_MUTANTS:
            if m not in cr.mutants_of(name, ora.do_cfg(g)):
                row.append(f"{m} -")
                continue
            mut = cr.oracle_run(ora, cell, inp, b, Mb, mutate=m)
            dl = float(np.abs(mut["latents"] - true["latents"]).max()) / bound
            di = float(np.abs(cr.image01(mut["image"]) - cr.image01(true["image"])).max())
            row.append(f"{m} {dl:.0f}|{di:.2f}")
            if not (dl >= cr.SEPARATION and di >= cr.SEPARATION * cr.IMG_TOL):
                bad.append((b, m, dl, di))
        print(f"[chain-matrix] {cr.cell_id(cell)} request {b} (bound {bound:.3g}): " + ", ".join(row))
    assert not bad, f"{cr.cell_id(cell)}: (request, mutant) within {cr.SEPARATION} bounds of the oracle: {bad}"


def test_variation_reaches_the_initial_latents():
    """The variation cells judge the blend into lat0: the oracle's initial latents with a variation differ from the plain draw,
    inside the paste window of the seed-resize and everywhere for the blend in place."""
    cell = ("variation", "a", 0)
    inp = cr.cell_inputs(cell)
    from sdlcm_amd.pipeline import draw_noise
    for b in range(2):
        l0 = draw_noise(inp["seeds"][b], 8, 8, 0)[0].numpy()
        got = cr.oracle_run(_oracle("a"), cell, inp, b, decode=False)["latents0"]
        assert got.shape == l0.shape and (got != l0).mean() > 0.5
