"""Prompt text of a request -> 77-token chunks with a weight per token ("Prompts").

Written after A1111's prompt handling from its documented behaviour, not from its source; equality with A1111 is unverified (there is
no A1111 here to compare with).  Pure Python: nothing on the parse path imports torch.

Grammar (``parse``):
  ``(x)``    the weight of x times 1.1            ``[x]``    the weight of x divided by 1.1
  ``(x:w)``  the weight of x times the float w    nesting multiplies
  ``\\(  \\)  \\[  \\]  \\\\``  literal characters
  an unclosed ``(`` / ``[`` applies x 1.1 / / 1.1 to everything after it; a closing bracket nothing opened is text
  adjacent runs of equal weight merge; ``BREAK`` as a whitespace-delimited word ends the current chunk
Not recognised -- text like any other: ``AND``, prompt editing ``[a:b:0.5]``, alternation ``[a|b]``, ``<lora:...>``, textual-inversion
names.

Chunks (``PromptChunker.chunk``): every run is tokenised without special tokens and each token carries its run's weight.  A chunk
holds 75 tokens.  When a token that is no comma arrives at a full chunk and the chunk's last comma has at most COMMA_BACKTRACK tokens
behind it, those tokens move to the next chunk; otherwise the chunk is simply closed.  A closed chunk is BOS + tokens + EOS, filled to 77
with the tokenizer's pad id, weight 1.0 on all three.  ``BREAK`` closes the current chunk whatever it holds (an empty one is a chunk of
padding); at the end of the text a chunk that holds tokens is closed, and so is an empty one if it would be the only chunk.
"""
from __future__ import annotations

import os
import re
import threading

CHUNK_TOKENS = 75
CHUNK_LEN = CHUNK_TOKENS + 2
COMMA_BACKTRACK = 20
ROUND, SQUARE = 1.1, 1.0 / 1.1

CTX_TAG = "ctx"                  # job / plan keys of a pass over n > 1 chunks end in (CTX_TAG, n)

BREAK = ("BREAK", -1.0)          # the marker parse() puts between runs: never a weight a run can have


def max_chunks() -> int:
    return max(1, int(os.environ.get("LCM_MAX_PROMPT_CHUNKS", "4") or 4))


_TOKEN = re.compile(r"\\[()\[\]\\]|\\|\(|\[|:\s*([+-]?(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?)\s*\)|\)|\]|[^\\()\[\]:]+|:")
_BREAK = re.compile(r"(?<!\S)BREAK(?!\S)")             # in the request's text: whitespace or an end of the text on either side


def parse(text: str):
    """-> [(text, weight) | BREAK]: the runs of the prompt in order, equal-weight neighbours merged.  The empty prompt is [("", 1.0)].
    BREAK is looked for in the text as the request wrote it, so ``(a)BREAK`` and ``a\\(BREAK`` hold the letters, not a break."""
    text = str(text)
    if "BREAK" not in text and not any(c in text for c in "()[]\\"):
        return [(text, 1.0)]                             # nothing to parse: one run (most requests)
    runs, round_open, square_open = [], [], []          # runs: [text, weight] | BREAK; *_open: index of the first run inside the bracket
    breaks = [m.span() for m in _BREAK.finditer(text)]

    def scale(start, f):
        for r in runs[start:]:
            if r is not BREAK:
                r[1] *= f

    for m in _TOKEN.finditer(text):
        tok = m.group(0)
        if tok[0] == "\\" and len(tok) == 2:
            runs.append([tok[1], 1.0])
        elif tok == "(":
            round_open.append(len(runs))
        elif tok == "[":
            square_open.append(len(runs))
        elif m.group(1) is not None and round_open:
            scale(round_open.pop(), float(m.group(1)))
        elif tok == ")" and round_open:
            scale(round_open.pop(), ROUND)
        elif tok == "]" and square_open:
            scale(square_open.pop(), SQUARE)
        else:                                            # text; also a closer with nothing open, a lone backslash, a colon
            at = m.start()                               # BREAK words inside this stretch of text cut it
            for a, b in breaks:
                if m.start() <= a and b <= m.end():
                    runs.append([text[at:a], 1.0])
                    runs.append(BREAK)
                    at = b
            runs.append([text[at:m.end()], 1.0])
    for start in round_open:
        scale(start, ROUND)
    for start in square_open:
        scale(start, SQUARE)
    out = []
    for r in runs:
        if r is BREAK:
            out.append(BREAK)
        elif r[0]:
            if out and out[-1] is not BREAK and out[-1][1] == r[1]:
                out[-1] = (out[-1][0] + r[0], r[1])
            else:
                out.append((r[0], r[1]))
    return out or [("", 1.0)]


class Chunked:
    """The chunks of one prompt: ids / weights are n lists of 77, n_tokens the prompt's token count without BOS / EOS / padding.
    Not changed after it is built (the chunker hands one object to every caller of a text)."""
    __slots__ = ("ids", "weights", "n_tokens", "_plain")

    def __init__(self, ids, weights, n_tokens):
        self.ids, self.weights, self.n_tokens = ids, weights, n_tokens
        self._plain = [all(w == 1.0 for w in ws) for ws in weights]

    @property
    def n(self) -> int:
        return len(self.ids)

    def plain(self, c: int) -> bool:
        """All weights of chunk c are exactly 1.0: its embedding is the text encoder's output as it is."""
        return self._plain[c]

    @property
    def weighted(self) -> bool:
        return not all(self._plain)


class PromptChunker:
    """parse + tokenise + chunk for one tokenizer.  The tokenizer gives ``encode_text(str) -> [int]`` (no special tokens, no
    truncation) and the ids ``bos``, ``eos``, ``pad``, ``comma`` (prompt._BpeTokenizer, clip.HashTokenizer).  Results are kept for the
    last few hundred prompt strings: a request's text is chunked once, for its key, and looked up for its pass."""

    CACHE = 512

    def __init__(self, tokenizer):
        self.tok = tokenizer
        self._cache = {}
        self._lock = threading.Lock()                # callers' threads (the key) and lane threads (the pass) share the cache

    def empty_chunk(self):
        t = self.tok
        return [t.bos, t.eos] + [t.pad] * CHUNK_TOKENS, [1.0] * CHUNK_LEN

    def count(self, text) -> int:
        """Number of chunks of ``text`` (raises like chunk()): always chunk()'s own count -- no shortcut on the text's length holds
        for a byte-level vocabulary, where one character can be several tokens."""
        return self.chunk(text).n

    def chunk(self, text) -> Chunked:
        text = "" if text is None else str(text)
        with self._lock:
            got = self._cache.get(text)
        if got is None:
            got = self._chunk(text)                   # outside the lock: two threads may chunk one text, to the same result
            with self._lock:
                if text not in self._cache and len(self._cache) >= self.CACHE:
                    del self._cache[next(iter(self._cache))]
                self._cache[text] = got
        if isinstance(got, Exception):
            raise RuntimeError(*got.args)
        return got

    def _chunk(self, text):
        t = self.tok
        ids, weights = [], []
        cur, cur_w, last_comma, total = [], [], -1, 0

        def close():
            nonlocal cur, cur_w, last_comma
            fill = CHUNK_TOKENS - len(cur)
            ids.append([t.bos] + cur + [t.eos] + [t.pad] * fill)
            weights.append([1.0] + cur_w + [1.0] * (fill + 1))
            cur, cur_w, last_comma = [], [], -1

        runs = parse(text)
        if len(runs) == 1 and runs[0] is not BREAK and runs[0][1] == 1.0:
            toks = [int(x) for x in t.encode_text(runs[0][0])]
            if len(toks) <= CHUNK_TOKENS:             # most requests: one plain chunk, nothing to cut or weigh
                return Chunked([[t.bos] + toks + [t.eos] + [t.pad] * (CHUNK_TOKENS - len(toks))], [[1.0] * CHUNK_LEN], len(toks))
        for run in runs:
            if run is BREAK:
                close()
                continue
            for tid in t.encode_text(run[0]):
                total += 1
                if len(cur) == CHUNK_TOKENS:
                    tail, tail_w = [], []
                    if tid != t.comma and last_comma != -1 and CHUNK_TOKENS - last_comma <= COMMA_BACKTRACK:
                        tail, tail_w = cur[last_comma:], cur_w[last_comma:]
                        cur, cur_w = cur[:last_comma], cur_w[:last_comma]
                    close()
                    cur, cur_w = tail, tail_w
                cur.append(int(tid))
                cur_w.append(float(run[1]))
                if tid == t.comma:
                    last_comma = len(cur)             # tokens up to and including the comma
        if cur or not ids:
            close()
        cap = max_chunks()
        if len(ids) > cap:
            return RuntimeError(f"prompt of {total} tokens needs {len(ids)} chunks of {CHUNK_TOKENS}: more than the cap of {cap} chunks "
                                f"(LCM_MAX_PROMPT_CHUNKS)")
        return Chunked(ids, weights, total)


def split_ctx(key):
    """A job key -> (the key without its ("ctx", n) ending, n); n = 1 when it has none."""
    if len(key) >= 2 and key[-2] == CTX_TAG:
        return tuple(key[:-2]), int(key[-1])
    return key, 1


def parse_clip_skip(req, num_layers: int) -> int:
    """The request's ``clip_skip`` (or ``override_settings["CLIP_stop_at_last_layers"]``), default 1: the hidden state after layer
    num_layers - (k - 1) goes through the final LayerNorm.  RuntimeError outside 1 .. num_layers."""
    k = getattr(req, "clip_skip", None)
    if k is None:
        ov = getattr(req, "override_settings", None)
        if isinstance(ov, dict):
            k = ov.get("CLIP_stop_at_last_layers")
    if k is None:
        return 1
    try:
        ki = int(k)
        ok = float(k) == ki
    except (TypeError, ValueError):
        ki, ok = 0, False
    if not ok or not 1 <= ki <= num_layers:
        raise RuntimeError(f"clip_skip {k!r} outside 1 .. {num_layers} (the text encoder's layers)")
    return ki


def negative_text(req) -> str:
    neg = getattr(req, "negative_prompt", None)
    return "" if neg is None else str(neg)
