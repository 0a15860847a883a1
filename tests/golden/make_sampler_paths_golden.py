"""Writes tests/golden/sampler_paths.json: what the sampler's host sequencing (LcmHipPipeline._enqueue) gives for every kind of
plan -- plain, classifier-free guidance, un-hoisted time embedding, ControlNet, refinement from scratch and from cached latents,
SDXL-style added embeddings -- and what the request sequencing around it gives for the two chained kinds, hires fix (plan,
hand-over, plan) and image-to-image (encoder stage, hand-over, plan), on 64x64-class requests with synthetic weights and fixed
seeds.  Run on an MI355X; it records the cases the file does not hold yet and carries the others over as they are:

    python tests/golden/make_sampler_paths_golden.py

Per case: the SHA-256 of ``rgb``, ``latents``, ``pool8`` (and ``xk`` / ``lowres_latents`` / ``init_latents``) of the graph-replayed
call, its ``xk_first`` / ``unet_evals`` / ``controlnet_evals``, and ``launches``: the kernel instantiations (indices into the file's
``kernels`` table) of ONE eager call of the same request, in launch order, as the library's own brackets report them (ops.profile_begin / profile_end).
LCM_AUTOTUNE=0 and the shipped plan table: the names depend on the table and the heuristics alone.

The file pins the bytes and the launch sequence across changes of the HOST code.  It is recorded on the commit BEFORE such a
change and must come out the same after it; tests/test_sampler_paths_gpu.py runs the same cases (``run_cases`` below) and
compares.  It is never re-recorded to make that test pass."""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

PATH = os.path.join(HERE, "sampler_paths.json")
DEV = "cuda:0"
SIZE = 64
HASHED = ("rgb", "latents", "pool8", "xk", "lowres_latents", "init_latents")
COUNTERS = ("xk_first", "unet_evals", "controlnet_evals")


def _sha(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _embeds(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 77, D, generator=g).half(), torch.randn(B, 77, D, generator=g).half()


@contextlib.contextmanager
def pipelines():
    """The three engines of the cases: SD1.5 LCM (guidance embedding), SD 2.x (v-prediction, no guidance embedding: guidance > 1
    is classifier-free guidance) -- each with its synthetic ControlNet and a lazy VAE encoder source (nothing is uploaded before
    the first image-to-image case) -- and the narrow SDXL-style set of
    tests/test_pipeline_gpu.py::test_sdxl_style_pipeline_parity."""
    import sdlcm_amd  # noqa: F401
    from sdlcm_amd import ops, weights
    from sdlcm_amd.config import SD2_UNET, SDXL_UNET, unet_config, vae_config
    from sdlcm_amd.pipeline import LcmHipPipeline
    from sdlcm_amd.scheduler import LCMSchedule, SD21_768_SCHEDULE
    old = os.environ.get("LCM_AUTOTUNE")
    os.environ["LCM_AUTOTUNE"] = "0"
    ops.plan_reset()                    # the shipped table: nothing an earlier tuning run of this process left behind
    vsd = weights.synthetic_vae()
    sd15 = LcmHipPipeline(weights.synthetic_unet(), vsd, device=DEV)
    sd15.set_controlnet(weights.synthetic_controlnet())
    sd2 = LcmHipPipeline(weights.synthetic_sd2_unet(), vsd, unet_config(SD2_UNET), device=DEV, schedule=LCMSchedule(**SD21_768_SCHEDULE))
    sd2.set_controlnet(weights.synthetic_controlnet(SD2_UNET), weights.controlnet_config(SD2_UNET))
    ucfg = unet_config(dict(SDXL_UNET, block_out_channels=(64, 128, 256), attention_head_dim=(1, 2, 4), cross_attention_dim=128,
                            transformer_layers_per_block=(1, 2, 2), addition_time_embed_dim=32,
                            projection_class_embeddings_input_dim=64 + 6 * 32))
    vcfg = vae_config(dict(block_out_channels=(64, 64, 128, 128), scaling_factor=0.13025))
    sdxl = LcmHipPipeline(weights.synthetic_state_dict(weights.unet_param_spec(ucfg), 0),
                          weights.synthetic_state_dict(weights.vae_param_spec(vcfg), 1), ucfg, vcfg, device=DEV)
    sd15.set_vae_encoder_source(weights.synthetic_vae_encoder)
    sd2.set_vae_encoder_source(weights.synthetic_vae_encoder)
    pipes = dict(sd15=sd15, sd2=sd2, sdxl=sdxl)
    try:
        yield pipes
    finally:
        for p in pipes.values():
            p.close()
        if old is None:
            os.environ.pop("LCM_AUTOTUNE", None)
        else:
            os.environ["LCM_AUTOTUNE"] = old


def _hints(B):
    import controlnet_reference as cr
    return np.stack([cr.test_hint(SIZE, SIZE, b) for b in range(B)])


def _pics(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _run(hip, call):
    """call(): one request on ``hip`` -> (record, result of the graph-replayed call).  The eager call of the same request runs
    second, on the request state the replay left in the plans' buffers, between the library's profile brackets; it must give
    the replay's bytes."""
    from sdlcm_amd import ops
    out = call()
    hip.use_graph = False
    try:
        ops.profile_begin()
        try:
            eager = call()
        finally:
            names = [n for n, _ in ops.profile_end()]
    finally:
        hip.use_graph = True
    rec = {k: _sha(out[k]) for k in HASHED if k in out}
    assert rec == {k: _sha(eager[k]) for k in HASHED if k in eager}, "the eager enqueue differs from the graph replay"
    rec.update({k: int(out[k]) for k in COUNTERS if k in out})
    rec["launches"] = names
    return rec, out


def _gen(hip, pe, seeds, steps, guidance=1.0, **kw):
    return _run(hip, lambda: hip.generate(pe, seeds, SIZE, SIZE, steps, guidance, **kw))


def _sampler_cases(pipes):
    """The cases of one generate() each; refine_cached_p3_from1_b2 needs the case before it, so these run as a group."""
    sd15, sd2, sdxl = pipes["sd15"], pipes["sd2"], pipes["sdxl"]
    res = {}
    pe1, _ = _embeds(1, 768, 5)
    pe2, _ = _embeds(2, 768, 6)
    pe3, _ = _embeds(3, 768, 7)
    res["plain_b1_4step"], _ = _gen(sd15, pe1, [42], 4, 1.5)
    res["plain_b3_1step"], _ = _gen(sd15, pe3, [1, 2, 3], 1)          # one step: the `last` step reads the dummy noise tensor
    q2, n2 = _embeds(2, 1024, 8)
    res["plain_cfg_sd2_b2"], _ = _gen(sd2, q2, [11, 12], 2, 5.0, negative_embeds=n2)
    sd15.unet.MAX_HOISTED_STEPS = 0                                     # per-step time_embed inside forward
    try:
        res["plain_unhoisted_b1_2step"], _ = _gen(sd15, pe1, [43], 2)
    finally:
        del sd15.unet.MAX_HOISTED_STEPS
    res["controlnet_b2"], _ = _gen(sd15, pe2, [21, 22], 2, control=(_hints(2), 0.75))
    q1, n1 = _embeds(1, 1024, 9)
    res["controlnet_cfg_sd2_b1"], _ = _gen(sd2, q1, [31], 2, 5.0, negative_embeds=n1, control=(_hints(1), 1.0))
    res["refine_scratch_p2_b2"], _ = _gen(sd15, pe2, [51, 52], 2, strength=0.5, passes=2)
    res["refine_scratch_cfg_sd2_p1_b1"], _ = _gen(sd2, q1, [61], 2, 5.0, negative_embeds=n1, strength=0.5, passes=1)
    res["refine_scratch_p3_b2"], full = _gen(sd15, pe2, [71, 72], 2, strength=0.5, passes=3)
    start = (1, [full["xk"][1, b].clone() for b in range(2)])
    res["refine_cached_p3_from1_b2"], part = _gen(sd15, pe2, [71, 72], 2, strength=0.5, passes=3, start=start)
    assert np.array_equal(part["rgb"], full["rgb"]), "the chain from cached x^1 differs from the chain from scratch"
    g = torch.Generator().manual_seed(8)
    pex = torch.randn(1, 77, 128, generator=g).half()
    added = (torch.randn(1, 64, generator=g).half(), torch.tensor([[64.0, 64.0, 0, 0, 64.0, 64.0]]))
    res["sdxl_plain_b1"], _ = _gen(sdxl, pex, [81], 2, added=added)
    res["sdxl_refine_p1_b1"], _ = _gen(sdxl, pex, [81], 2, added=added, strength=0.5, passes=1)
    return res


def _hires(hip, D, B, seed, steps, hires, guidance=1.0):
    pe, ne = _embeds(B, D, seed)
    seeds = [seed * 10 + b for b in range(B)]
    neg = ne if guidance > 1.0 else None
    return _run(hip, lambda: hip.generate(pe, seeds, SIZE, SIZE, steps, guidance, negative_embeds=neg, hires=hires))[0]


def _img2img(hip, D, B, seed, W, H, guidance=1.0):
    pe, ne = _embeds(B, D, seed)
    seeds, pics = [seed * 10 + b for b in range(B)], _pics(B, H, W, seed)
    neg = ne if guidance > 1.0 else None
    return _run(hip, lambda: hip.generate_img2img(pe, seeds, pics, W, H, 2, 0.5, guidance, negative_embeds=neg))[0]


# the chained request kinds, one independent case each; hires = (W2, H2, hr_steps, strength, mode)
CHAIN_CASES = {
    "hires_bilinear_b2": lambda p: _hires(p["sd15"], 768, 2, 101, 2, (96, 96, 2, 0.7, 0)),
    "hires_bicubic_cfg_sd2_b1": lambda p: _hires(p["sd2"], 1024, 1, 102, 2, (128, 128, 2, 0.7, 1), 5.0),
    "hires_nearest_1step_b3": lambda p: _hires(p["sd15"], 768, 3, 103, 1, (64, 64, 1, 0.7, 2)),
    "img2img_b2": lambda p: _img2img(p["sd15"], 768, 2, 104, 64, 64),
    "img2img_cfg_sd2_b1": lambda p: _img2img(p["sd2"], 1024, 1, 105, 64, 64, 5.0),
    "img2img_odd_b2": lambda p: _img2img(p["sd15"], 768, 2, 106, 72, 40),
}


def run_cases(pipes, have=()):
    """-> {case: record} of the cases not in ``have``, in the order of the list in the module docstring of
    tests/test_sampler_paths_gpu.py."""
    res = {} if "sdxl_refine_p1_b1" in have else _sampler_cases(pipes)       # the group's last case: all of it or none
    for name, case in CHAIN_CASES.items():
        if name not in have:
            res[name] = case(pipes)
    return res


def pack(res):
    """The file's form: the launch lists as indices into one table of kernel names."""
    table = sorted({n for r in res.values() for n in r["launches"]})
    idx = {n: i for i, n in enumerate(table)}
    return dict(kernels=table, cases={k: dict(r, launches=[idx[n] for n in r["launches"]]) for k, r in res.items()})


def unpack(doc):
    return {k: dict(r, launches=[doc["kernels"][i] for i in r["launches"]]) for k, r in doc["cases"].items()}


def main():
    res = {}
    if os.path.exists(PATH):                 # carried over unpacked: pack() sorts one name table, new names shift the indices
        with open(PATH) as f:
            res = unpack(json.load(f))
    with pipelines() as pipes:
        new = run_cases(pipes, have=set(res))
    res.update(new)
    doc = pack(res)
    line = lambda v: json.dumps(v, separators=(",", ":"))       # one kernel name / one case per line
    with open(PATH, "w") as f:
        f.write('{"kernels":[\n' + ",\n".join(line(n) for n in doc["kernels"]) + '\n],\n"cases":{\n')
        f.write(",\n".join(f"{line(k)}:{line(r)}" for k, r in doc["cases"].items()) + "\n}}\n")
    print(PATH, os.path.getsize(PATH), "bytes; recorded", {k: len(r["launches"]) for k, r in new.items()},
          "carried over", sorted(set(res) - set(new)))


if __name__ == "__main__":
    main()
