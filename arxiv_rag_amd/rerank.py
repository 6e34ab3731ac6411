"""Cross-encoder reranking on the MI355X: the second half of the upstream retrieval config (`use_reranking: true`,
`reranker_model: "cross-encoder/ms-marco-MiniLM-L-6-v2"`, 3-chunks/pipeline/config.yaml:63-69).

`HipCrossEncoder` mirrors `sentence_transformers.CrossEncoder` (`predict`, `rank`): a (query, passage) pair is tokenised as
"[CLS] query [SEP] passage [SEP]" (token type 1 from the passage on, `longest_first` truncation), run through the HIP encoder with
segment-aware embeddings, and scored by the pooler + classifier head on the final CLS row (`arx_encoder_score_pairs`).  There is no
CPU path.  By default a pair's logits are bitwise independent of the batch it was scored in; `low_latency=True` trades that for the
small-batch GEMM schedule (`arx_encoder_set_low_latency`).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .config import ACT_SIGMOID, CROSS_PRESETS, CrossEncoderConfig, cross_config_from_hf_dir
from .encoder import HipEncoder
from .weights import head_shapes


class HipCrossEncoder:
    """(query, passage) pairs -> relevance scores on one GPU."""

    def __init__(self, cfg: CrossEncoderConfig, state_dict: Dict[str, np.ndarray], tokenizer, device: Union[str, torch.device] = "cuda:0",
                 max_length: Optional[int] = None, low_latency: bool = False):
        """`state_dict`: the encoder's keys (as `weights.load_hf_dir` returns them) plus the head's (`weights.head_shapes`)."""
        enc = cfg.encoder
        self.cfg = cfg
        self.tokenizer = tokenizer
        self.max_length = min(int(max_length or enc.max_seq_length), enc.max_pos, 512)
        self.low_latency = bool(low_latency)
        hk = head_shapes(enc, cfg.n_labels)
        missing = [k for k in hk if k not in state_dict]
        if missing:
            raise KeyError(f"missing cross-encoder head weights {missing}")
        self.encoder = HipEncoder(enc, {k: v for k, v in state_dict.items() if k not in hk}, device=device,
                                  max_tokens=32 * self.max_length, max_seqs=32)
        self.device = self.encoder.device
        e = self.encoder
        # the [2, H] token-type table: row 0 carries the same f32 values the encoder's own type_emb pointer holds
        self._head_c = _lib.PairHeadC(n_labels=cfg.n_labels)
        self._head_c.type_emb = e._f32(state_dict["embeddings.token_type_embeddings.weight"]).data_ptr()
        self._head_c.pooler_w = e._f32(state_dict["pooler.dense.weight"]).data_ptr()
        self._head_c.pooler_b = e._f32(state_dict["pooler.dense.bias"]).data_ptr()
        self._head_c.cls_w = e._f32(state_dict["classifier.weight"]).data_ptr()
        self._head_c.cls_b = e._f32(state_dict["classifier.bias"]).data_ptr()
        torch.cuda.synchronize(self.device)
        self._head_on = None                  # (handle, capacity) the head was attached to (a capacity change builds a new handle)

    @classmethod
    def from_dir(cls, name: str, device="cuda:0", max_length: Optional[int] = None, low_latency: bool = False) -> "HipCrossEncoder":
        """Name or local BertForSequenceClassification directory (resolved by `hub.resolve_model_dir`; nothing is fetched)."""
        from .hub import resolve_model_dir
        from .tokenizer import WordPieceTokenizer
        from .weights import load_cross_encoder_dir
        d = resolve_model_dir(name)
        cfg = cross_config_from_hf_dir(d)
        preset = CROSS_PRESETS.get(name) or CROSS_PRESETS.get(name.split("/")[-1])
        if preset is not None and (preset.encoder.hidden, preset.encoder.layers, preset.n_labels) != \
                (cfg.encoder.hidden, cfg.encoder.layers, cfg.n_labels):
            raise ValueError(f"{d} does not hold a {name} checkpoint (shape mismatch)")
        sd, head = load_cross_encoder_dir(d, cfg.encoder, cfg.n_labels)
        tok = WordPieceTokenizer.from_dir(d, cfg.encoder, bert_pair=True)
        return cls(cfg, {**sd, **head}, tok, device=device, max_length=max_length, low_latency=low_latency)

    def close(self):
        self.encoder.close()

    # ---- device path ----------------------------------------------------------------------------
    def _prepare(self, total_tokens: int, n_seqs: int):
        e = self.encoder
        e._ensure_capacity(total_tokens, n_seqs)
        if self._head_on != (e._handle.value, e._cap):     # a new handle may reuse the old one's address, never its capacity
            _lib.check(e.lib.arx_encoder_set_pair_head(e._handle, C.byref(self._head_c)), "arx_encoder_set_pair_head")
            self._head_on = (e._handle.value, e._cap)
        if self.low_latency != e._low_latency:
            _lib.check(e.lib.arx_encoder_set_low_latency(e._handle, 1 if self.low_latency else 0), "arx_encoder_set_low_latency")
            e._low_latency = self.low_latency

    def score_device(self, ids: torch.Tensor, lens: torch.Tensor, seg_b: Optional[torch.Tensor], max_len: int, total_tokens: int,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Device int32 ids [B, S], lens [B], seg_b [B] (None: all token type 0) -> device f32 logits [B, n_labels] (current stream)."""
        B, S = ids.shape
        assert ids.dtype == torch.int32 and lens.dtype == torch.int32 and ids.is_contiguous() and lens.is_contiguous()
        assert seg_b is None or (seg_b.dtype == torch.int32 and seg_b.is_contiguous() and seg_b.numel() == B)
        self._prepare(total_tokens, B)
        if out is None:
            out = torch.empty((B, self.cfg.n_labels), dtype=torch.float32, device=self.device)
        e = self.encoder
        _lib.check(e.lib.arx_encoder_score_pairs(e._handle, ids.data_ptr(), S, lens.data_ptr(), None if seg_b is None else seg_b.data_ptr(),
                                                 B, max_len, total_tokens, out.data_ptr(), out.stride(0),
                                                 torch.cuda.current_stream().cuda_stream), "arx_encoder_score_pairs")
        return out

    def score_tokens(self, ids: np.ndarray, lens: np.ndarray, seg_b: np.ndarray, batch_size: int = 32) -> np.ndarray:
        """Host ids [n, W], lens [n], seg_b [n] -> f32 logits [n, n_labels] in input order.  Batches are length-sorted (descending) and
        packed; with the default schedule the rows do not depend on that grouping."""
        n = int(len(lens))
        out = np.zeros((n, self.cfg.n_labels), np.float32)
        if n == 0:
            return out
        lens = np.ascontiguousarray(lens, np.int32)
        order = np.argsort(-lens.astype(np.int64), kind="stable")
        dev_out = torch.empty((n, self.cfg.n_labels), dtype=torch.float32, device=self.device)
        bs = max(1, int(batch_size))
        for s0 in range(0, n, bs):
            idx = order[s0:s0 + bs]
            bl = lens[idx]
            ml = max(int(bl.max()), 1)
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device, non_blocking=True)
            self.score_device(to(ids[idx, :ml]), to(bl), to(seg_b[idx]), ml, max(int(bl.sum()), 1), out=dev_out[s0:s0 + len(idx)])
        out[order] = dev_out.cpu().numpy()
        return out

    def tap_hidden(self, ids: np.ndarray, lens: np.ndarray, seg_b: Optional[np.ndarray], layer: int) -> np.ndarray:
        """Parity tap across a pair scoring call: packed hidden state [sum(lens), H] f32 after `layer` (0 = embeddings)."""
        ids = np.ascontiguousarray(ids, np.int32); lens = np.ascontiguousarray(lens, np.int32)
        T = max(int(lens.sum()), 1)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        self._prepare(T, len(lens))
        e = self.encoder
        _lib.check(e.lib.arx_encoder_set_tap(e._handle, layer), "arx_encoder_set_tap")
        self.score_device(to(ids), to(lens), None if seg_b is None else to(seg_b), max(int(lens.max()), 1), T)
        dst = torch.empty((int(lens.sum()), self.cfg.encoder.hidden), dtype=torch.float32, device=self.device)
        _lib.check(e.lib.arx_encoder_debug_hidden(e._handle, layer, dst.data_ptr(), int(lens.sum()),
                                                  torch.cuda.current_stream().cuda_stream), "arx_encoder_debug_hidden")
        _lib.check(e.lib.arx_encoder_set_tap(e._handle, -1), "arx_encoder_set_tap")
        return dst.cpu().numpy()

    def last_cls_rows(self, n: int) -> torch.Tensor:
        """Parity tap: the f32 CLS rows [n, H] the head read in the last pair scoring call (device tensor)."""
        e = self.encoder
        dst = torch.empty((n, self.cfg.encoder.hidden), dtype=torch.float32, device=self.device)
        _lib.check(e.lib.arx_encoder_debug_cls(e._handle, dst.data_ptr(), n, torch.cuda.current_stream().cuda_stream),
                   "arx_encoder_debug_cls")
        return dst

    # ---- CrossEncoder-shaped API ----------------------------------------------------------------
    def tokenize_pairs(self, pairs: Sequence[Tuple[str, str]]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        return self.tokenizer.encode_pairs_packed(pairs, self.max_length)

    def predict(self, sentences, batch_size: int = 32, show_progress_bar=None, activation_fct=None, apply_softmax: bool = False,
                convert_to_numpy: bool = True, convert_to_tensor: bool = False, **_ignored):
        """`CrossEncoder.predict`: [(query, passage), ...] -> scores [n] (one label) or [n, n_labels], in input order.
        `activation_fct` (callable on a torch tensor) replaces the model's default activation (sigmoid for one label, identity
        otherwise); `apply_softmax` normalises over the labels when there are several.  A single pair gives a single score."""
        single = len(sentences) == 2 and isinstance(sentences[0], str)
        pairs = [sentences] if single else list(sentences)
        ids, lens, seg_b = self.tokenize_pairs(pairs)
        logits = torch.from_numpy(self.score_tokens(ids, lens, seg_b, batch_size=batch_size))
        if activation_fct is not None:
            scores = activation_fct(logits)
        elif self.cfg.activation == ACT_SIGMOID:
            scores = torch.sigmoid(logits)
        else:
            scores = logits
        if apply_softmax and scores.shape[1] > 1:
            scores = torch.softmax(scores, dim=1)
        if self.cfg.n_labels == 1:
            scores = scores[:, 0]
        if single:
            scores = scores[0]
        if convert_to_tensor or not convert_to_numpy:
            return scores
        return scores.numpy()

    def rank(self, query: str, documents: Sequence[str], top_k: Optional[int] = None, return_documents: bool = False,
             batch_size: int = 32, **kw) -> List[Dict]:
        """`CrossEncoder.rank`: [{"corpus_id", "score"[, "text"]}] sorted by score, descending; equal scores keep the lower corpus_id
        first."""
        if self.cfg.n_labels != 1:
            raise ValueError("rank() needs a single-label cross-encoder")
        documents = list(documents)
        if not documents:
            return []
        scores = np.asarray(self.predict([(query, d) for d in documents], batch_size=batch_size, convert_to_numpy=True, **kw),
                            np.float32).reshape(-1)
        order = np.lexsort((np.arange(len(documents)), -scores))
        out = []
        for j in order[:top_k] if top_k is not None else order:
            hit = {"corpus_id": int(j), "score": float(scores[j])}
            if return_documents:
                hit["text"] = documents[j]
            out.append(hit)
        return out


def rerank_candidates(score_pairs, queries: Sequence[str], cand: np.ndarray, texts: Dict[int, str], dist=None, group=None) -> Dict:
    """Score (query, candidate) pairs whose texts this process holds and merge over ranks.

    cand int [Q, N] global row ids (-1 = none), the same on every rank (the merged search answer); `texts` {row: text} for the rows
    this rank holds; `score_pairs([(query, text), ...]) -> scores [n]`.  Each rank scores only its own rows; the (query, row, score)
    triples are all-gathered over `group` (gloo, host objects) and merged.  -> {(qi, row): score} for every scored candidate."""
    trip = [(qi, int(j)) for qi in range(len(queries)) for j in cand[qi] if int(j) >= 0 and int(j) in texts]
    sc = np.asarray(score_pairs([(queries[qi], texts[j]) for qi, j in trip]), np.float32).reshape(-1) if trip else np.zeros(0, np.float32)
    mine = [(qi, j, float(s)) for (qi, j), s in zip(trip, sc)]
    if dist is not None and dist.get_world_size() > 1:
        parts: List = [None] * dist.get_world_size()
        dist.all_gather_object(parts, mine, group=group)
        mine = [t for p in parts for t in p]
    return {(qi, j): s for qi, j, s in mine}


def reorder_by_rerank(cand: np.ndarray, scores: Dict, top_k: int) -> List[List[Tuple[int, int, float]]]:
    """Per query: [(position in the cosine order, row, rerank score)] of the best `top_k` candidates by rerank score, descending; equal
    scores keep the cosine order."""
    out = []
    for qi in range(cand.shape[0]):
        hits = [(p, int(j), scores[(qi, int(j))]) for p, j in enumerate(cand[qi]) if (qi, int(j)) in scores]
        hits.sort(key=lambda h: (-h[2], h[0]))
        out.append(hits[:top_k])
    return out
