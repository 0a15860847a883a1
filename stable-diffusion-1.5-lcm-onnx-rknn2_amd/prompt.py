"""Prompt -> encoder_hidden_states [B, 77, 768] for the UNet cross-attention.

The text encoder itself runs on the HIP kernels (``clip.ClipTextHip``).  Tokenisation is host string work: the CLIP BPE
vocabulary of the checkpoint (``tokenizer/`` / ``tokenizer_2/``) through ``transformers.CLIPTokenizer`` -- padding /
truncation to 77 and int32 ids as backends/rknnlcm.py:305-324; the pad id is the directory's own (SDXL's second tokenizer
pads with id 0).  A single-file checkpoint carries no vocabulary (the reference's ``from_single_file`` fetches it,
backends/cuda_worker.py:78-85; there is no network here): point ``LCM_TOKENIZER_DIR`` at a directory holding ``tokenizer/``
(and ``tokenizer_2/`` for SDXL) or the vocabulary files themselves.  REAL text-encoder weights without a vocabulary are an
error -- hashed word ids would silently condition the image on garbage; only the synthetic-weight runs (no vocabulary
ships with the reference) use ``clip.HashTokenizer``, which just needs stable ids.
"""
from __future__ import annotations

import os

import torch

from . import ops
from .backends.prompt_syntax import PromptChunker
from .clip import ClipTextHip, HashTokenizer, load_clip_dir, synthetic_clip
from .config import TEXT_SEQ_LEN


class _BpeTokenizer:
    def __init__(self, d: str):
        from transformers import CLIPTokenizer
        self.tok = CLIPTokenizer.from_pretrained(d)
        # what backends/prompt_syntax.py needs: the ids a chunk is framed and filled with (the directory's own pad id, as the call
        # below pads) and the comma a chunk may be cut at
        self.bos, self.eos, self.pad = self.tok.bos_token_id, self.tok.eos_token_id, self.tok.pad_token_id
        self.comma = self.tok.get_vocab().get(",</w>", -1)

    def encode_text(self, text):
        """The ids of ``text`` without BOS / EOS, padding or truncation: what __call__ puts between BOS and EOS."""
        return self.tok.encode(str(text), add_special_tokens=False, truncation=False, verbose=False)

    def __call__(self, prompts):
        ids = self.tok(list(prompts), padding="max_length", max_length=TEXT_SEQ_LEN, truncation=True,
                       return_tensors="pt").input_ids
        return ids.to(torch.int32)


def make_tokenizer(ckpt_root, sub, vocab_size, real_weights):
    """The tokenizer that goes with a text encoder: ``<ckpt_root>/<sub>``, else ``$LCM_TOKENIZER_DIR/<sub>``, else
    ``$LCM_TOKENIZER_DIR`` itself (first tokenizer only); with synthetic weights and none of those, the hash stand-in."""
    from .lib import LcmHipError
    cands = [os.path.join(ckpt_root, sub)] if ckpt_root else []
    env = os.environ.get("LCM_TOKENIZER_DIR", "")
    if env:
        cands.append(os.path.join(env, sub))
        if sub == "tokenizer":
            cands.append(env)
    for d in cands:
        if os.path.isfile(os.path.join(d, "vocab.json")) or os.path.isfile(os.path.join(d, "tokenizer.json")):
            return _BpeTokenizer(d)
    if real_weights:
        raise LcmHipError(f"text encoder weights were loaded from a checkpoint but no CLIP vocabulary was found for '{sub}' "
                          f"(looked in {cands or ['<no checkpoint directory>']}): a single-file checkpoint does not carry one -- set "
                          f"LCM_TOKENIZER_DIR to a directory holding {sub}/vocab.json + merges.txt.  Refusing to tokenise real "
                          f"weights with hashed word ids.")
    return HashTokenizer(vocab_size)


class HipPromptEncoder:
    """prompts (list[str]) -> fp16 [B, 77, D] on the device, computed by the native CLIP text encoder."""

    def __init__(self, device, ckpt_root: str | None = None, clip_sd: dict | None = None, clip_cfg: dict | None = None):
        """clip_cfg: settings of a single-file text tower that its tensors do not show (SD 2.x: hidden_act="gelu",
        from weights.load_single_file's meta); the shapes give the rest."""
        te = os.path.join(ckpt_root, "text_encoder") if ckpt_root else None
        if clip_sd is not None:                      # text encoder carried inside a single-file checkpoint
            sd = clip_sd
            cfg = dict(num_hidden_layers=1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers.")),
                       hidden_size=sd["embeddings.token_embedding.weight"].shape[1],
                       vocab_size=sd["embeddings.token_embedding.weight"].shape[0],
                       intermediate_size=sd["encoder.layers.0.mlp.fc1.weight"].shape[0],
                       num_attention_heads=sd["embeddings.token_embedding.weight"].shape[1] // 64)
            cfg.update(clip_cfg or {})
            self.source = "single-file"
        elif te and os.path.isdir(te):
            sd, cfg = load_clip_dir(te)
            self.source = "checkpoint"
        else:
            sd, cfg = synthetic_clip(clip_cfg), clip_cfg
            self.source = "synthetic"
        self.enc = ClipTextHip(sd, cfg, device=device)
        self.tokenize = make_tokenizer(ckpt_root, "tokenizer", self.enc.cfg["vocab_size"], self.source != "synthetic")

        self.chunker = PromptChunker(self.tokenize)

    def __call__(self, prompts):
        return self.enc.forward(self.tokenize(prompts))

    @torch.inference_mode()
    def encode_chunked(self, texts, stops=None):
        """texts: one ``prompt_syntax.Chunked`` per output row, all of the same chunk count n; stops: the text encoder's stop layer
        per row (None: all layers).  -> (fp16 [len(texts), 77 n, D] on the device, chunks encoded).  All chunks of rows that share
        a stop layer go through CLIP as ONE batch (CLIP batches are batch-invariant); lcm_prompt_emphasis_f16 then writes the rows
        that carry weights into their slot of the result, and rows whose weights are all 1.0 are copied there (an exact skip,
        decided here on the host).  A batch of plain one-chunk rows with one stop layer is the call above: same launches, same
        bits."""
        enc = self.enc
        R, n, D = len(texts), texts[0].n, enc.D
        if any(t.n != n for t in texts):
            raise ValueError("encode_chunked: every row of a pass has the same number of chunks")
        stops = [enc.L if s is None else int(s) for s in (stops or [None] * R)]
        if n == 1 and len(set(stops)) == 1 and not any(t.weighted for t in texts):
            ids = torch.tensor([t.ids[0] for t in texts], dtype=torch.int32)
            return enc.forward(ids, stop=stops[0]), R
        out = torch.empty(R, n * TEXT_SEQ_LEN, D, dtype=torch.float16, device=enc.device)
        flat = out.reshape(R * n * TEXT_SEQ_LEN, D)
        for stop in sorted(set(stops), reverse=True):
            rows = [r for r in range(R) if stops[r] == stop]
            ids = torch.tensor([c for r in rows for c in texts[r].ids], dtype=torch.int32)
            z = enc.forward(ids, stop=stop, keep=True).reshape(len(rows) * n * TEXT_SEQ_LEN, D)
            w_d = None
            if any(texts[r].weighted for r in rows):
                w_d = torch.tensor([w for r in rows for c in texts[r].weights for w in c], dtype=torch.float32).to(enc.device, non_blocking=True)
            # spans of rows that are neighbours in the result and alike in carrying weights: one launch, or one copy, each
            i = 0
            while i < len(rows):
                j, wt = i + 1, texts[rows[i]].weighted
                while j < len(rows) and rows[j] == rows[j - 1] + 1 and texts[rows[j]].weighted == wt:
                    j += 1
                a, b = i * n * TEXT_SEQ_LEN, j * n * TEXT_SEQ_LEN
                dst = flat[rows[i] * n * TEXT_SEQ_LEN:(rows[i] + j - i) * n * TEXT_SEQ_LEN]
                if wt:
                    ops.prompt_emphasis(z[a:b], w_d[a:b], dst, (j - i) * n, TEXT_SEQ_LEN, D)
                else:
                    dst.copy_(z[a:b])
                i = j
        return out, R * n
