#!/usr/bin/env python3
"""Record tests/golden/parent_bits_entry_path.json: run ON A BUILD OF THE PARENT COMMIT, on the GPU.

  python tests/golden/make_parent_bits_entry_path.py <parent commit id> [output path]

sha256 of what every launch of tests/entry_path_cases.py writes (output, statistics slab count, statistics slabs) and of the
rgb / latents / pool8 of one 128x128 2-step request, as the parent commit's kernels compute them.  tests/test_entry_path_gpu.py
holds the tree's kernels to these bytes."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REQUEST = dict(width=128, height=128, steps=2, prompt_seed=5, seeds=[42], guidance_scale=1.0)


def request_hashes():
    import numpy as np
    import torch
    import sdlcm_amd  # noqa: F401
    from sdlcm_amd import weights
    from sdlcm_amd.pipeline import LcmHipPipeline
    pipe = LcmHipPipeline(weights.synthetic_unet(), weights.synthetic_vae(), device="cuda:0")
    pe = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(REQUEST["prompt_seed"])).to(torch.float16)
    out = pipe.generate(pe, REQUEST["seeds"], REQUEST["width"], REQUEST["height"], REQUEST["steps"], REQUEST["guidance_scale"])
    res = {}
    for k in ("rgb", "latents", "pool8"):
        a = out[k]
        a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
        res[k] = hashlib.sha256(a.tobytes()).hexdigest()
    return res


def main():
    import sdlcm_amd  # noqa: F401
    import entry_path_cases
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "parent_bits_entry_path.json")
    doc = {"parent_commit": commit, "cases": entry_path_cases.run_cases(), "request": dict(REQUEST, sha256=request_hashes())}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(doc['cases'])} cases")


if __name__ == "__main__":
    main()
