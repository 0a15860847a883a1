"""Writes tests/golden/oracle_controlnet_512_4step.npz: the CPU reference (tests/controlnet_reference.py, torch fp32) of one
ControlNet-conditioned 512x512 4-step request on the synthetic SD1.5 weights -- seed 42, the prompt embedding of the other
fixtures (randn seed 5, rounded to fp16), hint controlnet_reference.test_hint(512, 512), conditioning scale 1.0.

    python tests/golden/make_controlnet_golden.py

Stored: every pixel of the decoded image clamped to [0, 1], quantised to 10 bits (q = rint(1023 v): half a step is 4.9e-4, a
twentieth of the 1e-2 tolerance it is compared under; 16 bits would exceed the size the other fixtures keep) as the high 8 bits
``image_hi_dx`` uint8 [3,512,512] -- stored as differences along x modulo 256, which deflate better; cumulative sum modulo 256
restores them -- and the low 2 bits ``image_lo`` packed four to a byte, and the final latents as float16."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def save(out, q, latents):
    lo = (q & 3).astype(np.uint8).reshape(-1, 4)
    hi = (q >> 2).astype(np.int16)
    np.savez_compressed(out, image_hi_dx=np.diff(hi, axis=2, prepend=0).astype(np.uint8),
                        image_lo=(lo[:, 0] | lo[:, 1] << 2 | lo[:, 2] << 4 | lo[:, 3] << 6),
                        latents=latents, seed=np.int64(42), scale=np.float32(1.0))


def main():
    import sdlcm_amd  # noqa: F401
    from sdlcm_amd import weights
    import controlnet_reference as cr
    pe = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(5)).to(torch.float16).float()
    ora = cr.ControlNetPipelineOracle(weights.synthetic_unet(), weights.synthetic_vae(), weights.synthetic_controlnet())
    ref = ora(pe, 512, 512, 4, 1.0, 42, cr.test_hint(512, 512), 1.0)
    img = np.clip(ref["image"][0] / 2 + 0.5, 0, 1)
    out = os.path.join(HERE, "oracle_controlnet_512_4step.npz")
    save(out, np.rint(img * 1023).astype(np.uint16), ref["latents"][0].astype(np.float16))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
