"""Tokenizers.

* ``HFTokenizer`` wraps a HuggingFace ``tokenizer.json`` (the fast ``tokenizers`` library) or a
  SentencePiece ``tokenizer.model`` when a checkpoint directory provides one — the real vocabularies
  of duckdb-nsql (Llama-2 SentencePiece, 32k), Llama-3.2 (tiktoken-BPE, 128,256) and Mistral v0.3.
* ``ByteTokenizer`` is the self-contained fallback used with random-init weights (no checkpoint can
  be downloaded here): UTF-8 bytes mapped onto ids [n_special, n_special + 256) of the model's
  vocabulary, with the model's BOS/EOS ids and chat-template special tokens mapped to reserved ids
  so templated prompts round-trip.
"""
from __future__ import annotations

import json
import os
import re
from typing import Optional, Sequence

from .spec import ModelSpec


class ByteTokenizer:
    def __init__(self, vocab_size: int, bos_id: int = 1, eos_ids: Sequence[int] = (2,), offset: int = 3,
                 specials: Sequence[str] = ()):
        self.vocab_size = vocab_size
        self.bos_id = bos_id
        self.eos_ids = tuple(eos_ids)
        self.offset = offset
        assert offset + 256 <= vocab_size or vocab_size >= 259, "vocab too small for byte fallback"
        # special strings (e.g. "<|eot_id|>") get reserved ids after the byte range
        self.special_to_id = {}
        nxt = offset + 256
        for s in specials:
            if nxt < vocab_size:
                self.special_to_id[s] = nxt
                nxt += 1
        self.id_to_special = {v: k for k, v in self.special_to_id.items()}

    def encode(self, text: str, add_bos: bool = True) -> list[int]:
        ids = [self.bos_id] if add_bos else []
        i = 0
        specials = sorted(self.special_to_id, key=len, reverse=True)
        while i < len(text):
            for s in specials:
                if text.startswith(s, i):
                    ids.append(self.special_to_id[s])
                    i += len(s)
                    break
            else:
                ids.extend(b + self.offset for b in text[i].encode("utf-8"))
                i += 1
        return ids

    def decode(self, ids: Sequence[int], skip_special: bool = True) -> str:
        out = bytearray()
        text = []
        for t in ids:
            t = int(t)
            if self.offset <= t < self.offset + 256:
                out.append(t - self.offset)
            elif t in self.id_to_special and not skip_special:
                text.append(out.decode("utf-8", errors="replace"))
                out = bytearray()
                text.append(self.id_to_special[t])
        text.append(out.decode("utf-8", errors="replace"))
        return "".join(text)


class HFTokenizer:
    def __init__(self, path: str, bos_id: Optional[int] = None, eos_ids: Sequence[int] = ()):
        tj = os.path.join(path, "tokenizer.json")
        sp = os.path.join(path, "tokenizer.model")
        self._sp = None
        self._tk = None
        if os.path.exists(tj):
            from tokenizers import Tokenizer

            self._tk = Tokenizer.from_file(tj)
        elif os.path.exists(sp):
            import sentencepiece as spm

            self._sp = spm.SentencePieceProcessor(model_file=sp)
        else:
            raise FileNotFoundError(f"no tokenizer.json / tokenizer.model in {path}")
        self.bos_id = bos_id if bos_id is not None else (self._sp.bos_id() if self._sp else 1)
        self.eos_ids = tuple(eos_ids) or ((self._sp.eos_id(),) if self._sp else (2,))

    @classmethod
    def from_tokenizer(cls, tk, bos_id: int = 1, eos_ids: Sequence[int] = (2,)) -> "HFTokenizer":
        """Wrap an already built ``tokenizers.Tokenizer`` (a GGUF file's vocabulary, ``tokenizer_from_gguf``)."""
        self = cls.__new__(cls)
        self._sp, self._tk = None, tk
        self.bos_id, self.eos_ids = bos_id, tuple(eos_ids) or (2,)
        return self

    def encode(self, text: str, add_bos: bool = True) -> list[int]:
        if self._tk is not None:
            ids = self._tk.encode(text, add_special_tokens=False).ids
        else:
            ids = self._sp.encode(text)
        return ([self.bos_id] if add_bos else []) + list(ids)

    def decode(self, ids: Sequence[int], skip_special: bool = True) -> str:
        ids = [int(i) for i in ids]
        if self._tk is not None:
            return self._tk.decode(ids, skip_special_tokens=skip_special)
        return self._sp.decode(ids)


LLAMA3_SPECIALS = ("<|begin_of_text|>", "<|start_header_id|>", "<|end_header_id|>", "<|eot_id|>",
                   "<|end_of_text|>")
MISTRAL_SPECIALS = ("[INST]", "[/INST]")


def _sp_merges(tokens, scores) -> list:
    """The BPE merges of a SentencePiece vocabulary that carries only scores (Llama-2 GGUF files), as "left right"
    strings, best first: the rule of transformers' GGUF tokenizer skeleton, with set lookups (its list lookups take
    minutes at 32k pieces)."""
    rank = {t: i for i, t in enumerate(tokens)}
    score = {t: scores[i] for i, t in enumerate(tokens)}
    merges = []
    for piece, sc in score.items():
        local = [(piece[:i], piece[i:]) for i in range(1, len(piece)) if piece[:i] in rank and piece[i:] in rank]
        local.sort(key=lambda lr: (score[lr[0]], score[lr[1]]), reverse=True)
        merges.extend((l, r, sc) for l, r in local if " " not in l and " " not in r)
    merges.sort(key=lambda m: m[2], reverse=True)
    return [f"{l} {r}" for l, r, _ in merges]


def tokenizer_from_gguf(spec: ModelSpec, tokdict: dict) -> HFTokenizer:
    """The tokenizer a GGUF file describes in its ``tokenizer.ggml.*`` metadata (models/gguf.py tokenizer_dict),
    built by transformers' GGUF converter of the llama architecture: a ``llama`` (SentencePiece-style, scores) or a
    ``gpt2`` (byte-level BPE, merges) vocabulary."""
    from transformers.integrations.ggml import convert_gguf_tokenizer  # lazy: only GGUF loads without tokenizer files

    td = dict(tokdict)
    kind = td.get("tokenizer_type")
    if kind == "llama" and "merges" not in td and "scores" in td:
        td["merges"] = _sp_merges(td["tokens"], td["scores"])
    tk, _ = convert_gguf_tokenizer("llama", td)  # the architecture's converter reads tokenizer_type itself
    return HFTokenizer.from_tokenizer(tk, spec.bos_id, spec.eos_ids)


def tokenizer_for(spec: ModelSpec, path: Optional[str] = None, gguf_tokenizer: Optional[dict] = None):
    # a checkpoint directory with its tokenizer files: the real tokenizer; weights-only directories
    # fall back to the byte tokenizer below.  A GGUF file: tokenizer files beside it first, else the vocabulary in its
    # own metadata (``gguf_tokenizer``); a vocabulary that cannot be built falls back too, with a warning
    if path and os.path.isfile(path):
        path = os.path.dirname(os.path.abspath(path))
    if path and any(os.path.exists(os.path.join(path, f)) for f in ("tokenizer.json", "tokenizer.model")):
        return HFTokenizer(path, spec.bos_id, spec.eos_ids)
    if gguf_tokenizer:
        try:
            return tokenizer_from_gguf(spec, gguf_tokenizer)
        except Exception as e:  # noqa: BLE001 - any converter failure: the load goes on with the byte tokenizer
            import warnings

            warnings.warn(f"GGUF tokenizer ({gguf_tokenizer.get('tokenizer_type')!r}) could not be built "
                          f"({type(e).__name__}: {e}); falling back to the byte tokenizer")
    specials = LLAMA3_SPECIALS if spec.template == "llama3" else MISTRAL_SPECIALS if spec.template == "mistral" else ()
    tok = ByteTokenizer(spec.vocab_size, bos_id=spec.bos_id if spec.bos_id < spec.vocab_size else 1,
                        eos_ids=[e for e in spec.eos_ids if e < spec.vocab_size] or [2], specials=specials)
    if spec.template == "llama3":  # the end-of-turn marker terminates generation
        eot = tok.special_to_id.get("<|eot_id|>")
        if eot is not None:
            tok.eos_ids = tuple(sorted(set(tok.eos_ids) | {eot}))
    return tok


# ----------------------------------------------------------------------------------- token byte table
def _gpt2_unicode_to_byte() -> dict:
    """Inverse of the GPT-2 byte -> printable-unicode map that byte-level BPE vocabularies are written in."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[chr(b)] = b
        else:
            table[chr(256 + n)] = b
            n += 1
    return table


_BYTE_PIECE = re.compile(r"^<0x([0-9A-Fa-f]{2})>$")


def _sp_piece_bytes(piece: str) -> bytes:
    """SentencePiece rule: ``<0xNN>`` is one byte, ``\u2581`` a space."""
    m = _BYTE_PIECE.match(piece)
    if m:
        return bytes([int(m.group(1), 16)])
    return piece.replace("\u2581", " ").encode("utf-8")


def _has_type(node, name: str) -> bool:
    if isinstance(node, dict):
        return node.get("type") == name or any(_has_type(v, name) for v in node.values())
    if isinstance(node, list):
        return any(_has_type(v, name) for v in node)
    return False


def token_bytes(tokenizer, vocab_size: Optional[int] = None):
    """The bytes every vocabulary id decodes to, in CSR form: ``(offsets int32 [V + 1], blob uint8 [offsets[V]])``
    (numpy).  Special, added, control and unknown ids map to zero bytes.  ``vocab_size`` (the model's, which may
    exceed the tokenizer's) pads the table with zero-byte ids.  What regex-constrained decoding walks its DFA over."""
    import numpy as np

    pieces: dict = {}
    if isinstance(tokenizer, ByteTokenizer):
        n = tokenizer.vocab_size
        for b in range(256):
            if tokenizer.offset + b < n:
                pieces[tokenizer.offset + b] = bytes([b])
    elif getattr(tokenizer, "_tk", None) is not None:
        tk = tokenizer._tk
        cfg = json.loads(tk.to_str())
        byte_level = _has_type(cfg.get("pre_tokenizer"), "ByteLevel") or _has_type(cfg.get("decoder"), "ByteLevel")
        u2b = _gpt2_unicode_to_byte() if byte_level else None
        added = set(tk.get_added_tokens_decoder())
        vocab = tk.get_vocab(with_added_tokens=True)
        n = max(vocab.values(), default=-1) + 1
        for piece, i in vocab.items():
            if i in added:
                continue
            if u2b is not None:
                if all(ch in u2b for ch in piece):
                    pieces[i] = bytes(u2b[ch] for ch in piece)
            else:
                pieces[i] = _sp_piece_bytes(piece)
    elif getattr(tokenizer, "_sp", None) is not None:
        sp = tokenizer._sp
        n = sp.get_piece_size()
        for i in range(n):
            if sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i):
                continue
            pieces[i] = _sp_piece_bytes(sp.id_to_piece(i))
    else:
        raise TypeError(f"token_bytes: unsupported tokenizer {type(tokenizer).__name__}")
    for e in (getattr(tokenizer, "bos_id", None), *getattr(tokenizer, "eos_ids", ())):
        pieces.pop(e, None)
    V = max(n, int(vocab_size or 0))
    lens = np.zeros(V + 1, dtype=np.int64)
    for i, b in pieces.items():
        lens[i + 1] = len(b)
    offsets = np.cumsum(lens).astype(np.int32)
    blob = np.frombuffer(b"".join(pieces[i] for i in sorted(pieces)), dtype=np.uint8).copy()
    assert int(offsets[-1]) == blob.shape[0]
    return offsets, blob
