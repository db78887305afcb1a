"""BERT-base encoder (12L/768H/12A, seq 128) for the streaming-inference
processor — random-init weights, bf16 end-to-end. Every hot op is a
hand-written gfx950 kernel: fused GEMM+bias(+GELU), fused attention
(QK^T·softmax·V in one launch), fused residual-add LayerNorm.

BASELINE.json config 5: generate → BERT-base inference, seq_len=128, bf16
MFMA, data-parallel across GPUs.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from ..ops import nn as opsnn


class BertConfig:
    def __init__(self, vocab_size=30528, hidden=768, layers=12, heads=12,
                 ff=3072, seq_len=128, num_labels=2):
        self.vocab_size = vocab_size
        self.hidden = hidden
        self.layers = layers
        self.heads = heads
        self.ff = ff
        self.seq_len = seq_len
        self.num_labels = num_labels
        self.head_dim = hidden // heads


class BertEncoder:
    def __init__(self, config: Optional[BertConfig] = None,
                 device: torch.device = torch.device("cpu"), seed: int = 42):
        self.cfg = config or BertConfig()
        self.device = torch.device(device)
        c = self.cfg
        gen = torch.Generator().manual_seed(seed)

        def w(*shape, std=0.02):
            return (torch.randn(*shape, generator=gen) * std).to(
                self.device, torch.bfloat16)

        def bias(n):
            return torch.zeros(n, device=self.device, dtype=torch.float32)

        def ones(n):
            return torch.ones(n, device=self.device, dtype=torch.float32)

        self.tok_emb = w(c.vocab_size, c.hidden)
        self.pos_emb = w(c.seq_len, c.hidden)
        self.emb_gamma, self.emb_beta = ones(c.hidden), bias(c.hidden)
        self.layers = []
        for _ in range(c.layers):
            self.layers.append({
                "wqkv": w(3 * c.hidden, c.hidden, std=0.02),
                "bqkv": bias(3 * c.hidden),
                "wo": w(c.hidden, c.hidden),
                "bo": bias(c.hidden),
                "ln1_g": ones(c.hidden), "ln1_b": bias(c.hidden),
                "w1": w(c.ff, c.hidden), "b1": bias(c.ff),
                "w2": w(c.hidden, c.ff), "b2": bias(c.hidden),
                "ln2_g": ones(c.hidden), "ln2_b": bias(c.hidden),
            })
        self.pool_w = w(c.hidden, c.hidden)
        self.pool_b = bias(c.hidden)
        self.cls_w = w(c.num_labels, c.hidden)
        self.cls_b = bias(c.num_labels)
        self._scale = 1.0 / math.sqrt(c.head_dim)
        # hipGraph capture: the encoder is shape-static per (B, S), so the
        # whole forward (~80 kernel launches) replays as ONE graph launch
        import os as _os
        self.use_graph = _os.environ.get("ARKFLOW_BERT_GRAPH", "1") != "0"
        # (B, S) → (graph, static_ids, static_logits); masked forwards are
        # keyed ("masked", B rounded up to 8, S) → (graph, static_ids,
        # static_lens, static_logits)
        self._graphs = {}

    # -------------------------------------------------------------- forward
    def forward(self, token_ids: torch.Tensor,
                lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """token_ids: [B, S] int64 → logits [B, num_labels] float32.

        lengths: optional int [B] tensor; sequence b then consists of its
        first lengths[b] tokens only, and logits row b depends on nothing
        else in the batch (a length of 0 gives finite, meaningless logits)."""
        if self.use_graph and self.device.type == "cuda":
            if lengths is None:
                return self._forward_graphed(token_ids)
            return self._forward_graphed_masked(token_ids, lengths)
        return self._forward_eager(token_ids, lengths)

    def _capture(self, static_ids, static_lens=None):
        """Warm up on a side stream (allocator settles), then capture one
        eager forward over the static buffers. Returns (graph, logits)."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._forward_eager(static_ids, static_lens)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            static_logits = self._forward_eager(static_ids, static_lens)
        return graph, static_logits

    def _forward_graphed(self, token_ids: torch.Tensor) -> torch.Tensor:
        key = tuple(token_ids.shape)
        entry = self._graphs.get(key)
        if entry is None:
            static_ids = token_ids.to(self.device).clone()
            graph, static_logits = self._capture(static_ids)
            entry = (graph, static_ids, static_logits)
            self._graphs[key] = entry
        graph, static_ids, static_logits = entry
        static_ids.copy_(token_ids.to(self.device))
        graph.replay()
        return static_logits

    def _forward_graphed_masked(self, token_ids: torch.Tensor,
                                lengths: torch.Tensor) -> torch.Tensor:
        """One graph per (B rounded up to a multiple of 8, S): a stream whose
        document count changes from batch to batch then replays a handful of
        graphs and does not capture one per distinct B. The extra rows have
        ids 0 and length 0; their logits are dropped."""
        B, S = token_ids.shape
        Bp = -(-B // 8) * 8
        key = ("masked", Bp, S)
        entry = self._graphs.get(key)
        if entry is None:
            static_ids = torch.zeros(Bp, S, dtype=torch.int64,
                                     device=self.device)
            static_lens = torch.zeros(Bp, dtype=torch.int32,
                                      device=self.device)
            graph, static_logits = self._capture(static_ids, static_lens)
            entry = (graph, static_ids, static_lens, static_logits)
            self._graphs[key] = entry
        graph, static_ids, static_lens, static_logits = entry
        static_ids[:B].copy_(token_ids.to(self.device))
        static_ids[B:].zero_()
        static_lens[:B].copy_(lengths.to(self.device))
        static_lens[B:].zero_()
        graph.replay()
        return static_logits[:B].clone()

    def _forward_eager(self, token_ids: torch.Tensor,
                       lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        c = self.cfg
        B, S = token_ids.shape
        ids = token_ids.to(self.device)
        lens = None if lengths is None else \
            lengths.to(self.device, torch.int32).contiguous()
        x = self.tok_emb[ids.reshape(-1) % c.vocab_size].reshape(B, S, c.hidden)
        x = x + self.pos_emb[:S].unsqueeze(0)
        x = opsnn.layernorm_bf16(x.contiguous(), self.emb_gamma, self.emb_beta)
        for ly in self.layers:
            x = self._layer(x, ly, B, S, lens)
        cls = x[:, 0, :].contiguous()  # [B, hidden]
        pooled = opsnn.linear_bf16(cls, self.pool_w, self.pool_b, act="none")
        pooled = torch.tanh(pooled.float()).to(torch.bfloat16)
        logits = opsnn.linear_bf16(pooled, self.cls_w, self.cls_b)
        return logits.float()

    def _layer(self, x: torch.Tensor, ly: dict, B: int, S: int,
               lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        c = self.cfg
        h = c.hidden
        x2 = x.reshape(B * S, h)
        qkv = opsnn.linear_bf16(x2, ly["wqkv"], ly["bqkv"])  # [B*S, 3h]
        qkv = qkv.reshape(B, S, 3, c.heads, c.head_dim)
        # strided attention straight off the QKV tensor (no transposes)
        # (lens: rows ≥ lens[b] of sequence b are padding — masked as keys,
        # written as 0 as queries)
        attn = opsnn.attention_qkv_bf16(qkv, self._scale,
                                        lens).reshape(B * S, h)
        proj = opsnn.linear_bf16(attn, ly["wo"], ly["bo"])
        x = opsnn.layernorm_bf16(proj.reshape(B, S, h), ly["ln1_g"],
                                 ly["ln1_b"], residual=x)
        ff = opsnn.linear_bf16(x.reshape(B * S, h), ly["w1"], ly["b1"],
                               act="gelu")
        ff2 = opsnn.linear_bf16(ff, ly["w2"], ly["b2"])
        x = opsnn.layernorm_bf16(ff2.reshape(B, S, h), ly["ln2_g"],
                                 ly["ln2_b"], residual=x)
        return x
