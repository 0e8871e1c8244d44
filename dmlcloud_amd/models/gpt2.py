"""GPT-2 small for the synthetic-token benchmark config (BASELINE.json).

Self-contained GPT-2 (124M): learned positional embeddings, pre-LN
blocks, GELU MLP, tied LM head. Attention goes through
ops.fused_attn.sdpa: the project's MFMA flash-attention kernels for bf16
device tensors with head dim 64 (GPT-2 small) or 128, torch SDPA otherwise.

Packed sequences: `GPT2.forward(idx, targets, doc_ids=...)` takes an
integer [B, T] tensor whose runs of equal values are the documents packed
into each row. Attention then stays inside a document and the learned
positions restart at every document start, so each document is computed
exactly as if it were alone in its row.

Grouped-query attention: `GPT2Config.n_kv_head` (a divisor of `n_head`)
gives K and V fewer heads than Q. `c_attn` then projects to
`n_embd + 2 * n_kv_head * head_dim` features and query head h reads K/V
head h // (n_head // n_kv_head). `None` (or `n_head`) is plain GPT-2,
unchanged.

Sampling: `GPT2.generate(idx, max_new_tokens)` prefills a per-layer K/V
cache (`init_cache`) from the prompt through the same `sdpa` path as
training and then decodes one token per `decode_step` through
ops.fused_attn.sdpa_kvcache, the split-KV decode kernels. The cache
lengths live on the device and are advanced there, so a step has no host
sync. `GPT2.extend(idx, cache)` appends a whole chunk of tokens to a cache
that may already hold some (chunked prefill, `generate(prefill_chunk=c)`,
the next turn of a conversation) through the same op with Nq = T.

Paged cache: `init_paged_cache` (or `generate(page_size=p)`) keeps K and V
in pools of fixed-size pages named by a per-row block table
(`PagedKVCache`) in place of one dense tensor per layer. `prefill`,
`decode_step` and `extend` take either cache type; on the paged one the new
rows are written by `ops.fused_attn.kvcache_append` (one launch per layer)
and read by `sdpa_kvcache(block_table=...)`. The table is fixed when the
cache is made; a free list or growth is the caller's.

FP8 cache: `init_cache(dtype=torch.float8_e4m3fn)`, `init_paged_cache(dtype=
...)` or `generate(kv_dtype=...)` keep K and V as e4m3 bytes with per-layer,
per-K/V-head fp32 scales (`cache.k_scale[layer]`, `cache.v_scale[layer]`,
[n_kv_head], ones by default, assignable; calibration is the caller's). Every
write then goes through `kvcache_append`, which quantises, dense cache
included, and every read through `sdpa_kvcache(k_scale=, v_scale=)`; `prefill`
still attends the prompt's own unquantised K/V.
"""

import math
from dataclasses import dataclass
from typing import List, Optional

import torch
from torch import nn
from torch.nn import functional as F

from ..ops.fused_attn import document_starts, kvcache_append, sdpa, sdpa_kvcache
from ..ops.fused_ln import LayerNorm
from ..ops.fused_loss import cross_entropy


@dataclass
class GPT2Config:
    vocab_size: int = 50257
    n_positions: int = 1024
    n_embd: int = 768
    n_layer: int = 12
    n_head: int = 12
    dropout: float = 0.0
    n_kv_head: Optional[int] = None  # K/V heads (GQA); None = n_head


class CausalSelfAttention(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        assert cfg.n_embd % cfg.n_head == 0
        self.n_head = cfg.n_head
        self.n_kv_head = cfg.n_head if cfg.n_kv_head is None else cfg.n_kv_head
        assert self.n_kv_head >= 1 and cfg.n_head % self.n_kv_head == 0, 'n_kv_head must divide n_head'
        self.kv_dim = self.n_kv_head * (cfg.n_embd // cfg.n_head)  # n_embd unless grouped
        self.c_attn = nn.Linear(cfg.n_embd, cfg.n_embd + 2 * self.kv_dim)
        self.c_proj = nn.Linear(cfg.n_embd, cfg.n_embd)

    def forward(self, x, doc_start=None):
        B, T, C = x.shape
        qkv = self.c_attn(x)
        # strided views into qkv, handed to sdpa without a copy; with
        # n_kv_head < n_head, k and v are [B, n_kv_head, T, hd]
        q, k, v = qkv.split([C, self.kv_dim, self.kv_dim], dim=2)
        q = q.view(B, T, self.n_head, C // self.n_head).transpose(1, 2)
        k = k.view(B, T, self.n_kv_head, C // self.n_head).transpose(1, 2)
        v = v.view(B, T, self.n_kv_head, C // self.n_head).transpose(1, 2)
        # custom MFMA flash attention on bf16, D = 64 or 128 (ops/fused_attn.py);
        # beats AOTriton fwd+bwd combined at this shape — falls back to
        # torch SDPA otherwise
        y = sdpa(q, k, v, causal=True) if doc_start is None else sdpa(q, k, v, causal=True, doc_start=doc_start)
        y = y.transpose(1, 2).reshape(B, T, C)
        return self.c_proj(y)

    def _heads(self, x):
        B, T, C = x.shape
        q, k, v = self.c_attn(x).split([C, self.kv_dim, self.kv_dim], dim=2)
        q = q.view(B, T, self.n_head, C // self.n_head).transpose(1, 2)
        k = k.view(B, T, self.n_kv_head, C // self.n_head).transpose(1, 2)
        v = v.view(B, T, self.n_kv_head, C // self.n_head).transpose(1, 2)
        return q, k, v

    def prefill(self, x, k_cache, v_cache):
        """forward(x) that also copies the prompt's K/V into cache rows 0..T-1."""
        B, T, C = x.shape
        q, k, v = self._heads(x)
        k_cache[:, :, :T] = k
        v_cache[:, :, :T] = v
        return self.c_proj(sdpa(q, k, v, causal=True).transpose(1, 2).reshape(B, T, C))

    def decode(self, x, k_cache, v_cache, kv_len, batch, pos):
        """One new token per row, x [B, 1, C]: its K/V go to cache row
        pos[b] = kv_len[b] - 1 (an indexed device write), then it attends
        the kv_len[b] valid rows."""
        B, _, C = x.shape
        q, k, v = self._heads(x)
        k_cache[batch, :, pos] = k[:, :, 0]
        v_cache[batch, :, pos] = v[:, :, 0]
        y = sdpa_kvcache(q, k_cache, v_cache, kv_len, causal=True)
        return self.c_proj(y.transpose(1, 2).reshape(B, 1, C))

    def extend(self, x, k_cache, v_cache, kv_len, batch, rows):
        """T new tokens per row, x [B, T, C]: their K/V go to cache rows
        rows[b, t] = kv_len[b] - T + t (one indexed device write per
        tensor), then token t attends cache rows 0..rows[b, t]."""
        B, T, C = x.shape
        q, k, v = self._heads(x)
        # index result [B, T, n_kv_head, hd]: the layout of k before its transpose
        k_cache[batch, :, rows] = k.transpose(1, 2)
        v_cache[batch, :, rows] = v.transpose(1, 2)
        y = sdpa_kvcache(q, k_cache, v_cache, kv_len, causal=True)
        return self.c_proj(y.transpose(1, 2).reshape(B, T, C))

    def prefill_paged(self, x, k_pool, v_pool, kv_len, block_table, k_scale=None, v_scale=None):
        """forward(x) that also writes the prompt's K/V through the block
        table (kv_len already holds T for every row). block_table None: a
        dense fp8 cache, which is written by the same launch."""
        B, T, C = x.shape
        q, k, v = self._heads(x)
        kvcache_append(k, v, k_pool, v_pool, kv_len, block_table, k_scale=k_scale, v_scale=v_scale)
        return self.c_proj(sdpa(q, k, v, causal=True).transpose(1, 2).reshape(B, T, C))

    def extend_paged(self, x, k_pool, v_pool, kv_len, block_table, k_scale=None, v_scale=None):
        """T >= 1 new tokens per row, x [B, T, C], on a paged cache: their K/V
        go to logical rows kv_len[b] - T + t of the row's pages (one launch),
        then token t attends logical rows 0..kv_len[b] - T + t. block_table
        None: a dense fp8 cache, the same two calls."""
        B, T, C = x.shape
        q, k, v = self._heads(x)
        kvcache_append(k, v, k_pool, v_pool, kv_len, block_table, k_scale=k_scale, v_scale=v_scale)
        y = sdpa_kvcache(
            q, k_pool, v_pool, kv_len, causal=True, block_table=block_table, k_scale=k_scale, v_scale=v_scale
        )
        return self.c_proj(y.transpose(1, 2).reshape(B, T, C))


class Block(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.ln_1 = LayerNorm(cfg.n_embd)
        self.attn = CausalSelfAttention(cfg)
        self.ln_2 = LayerNorm(cfg.n_embd)
        self.mlp = nn.Sequential(
            nn.Linear(cfg.n_embd, 4 * cfg.n_embd),
            nn.GELU(approximate='tanh'),
            nn.Linear(4 * cfg.n_embd, cfg.n_embd),
        )

    def forward(self, x, doc_start=None):
        x = x + self.attn(self.ln_1(x), doc_start)
        x = x + self.mlp(self.ln_2(x))
        return x

    def prefill(self, x, k_cache, v_cache):
        x = x + self.attn.prefill(self.ln_1(x), k_cache, v_cache)
        return x + self.mlp(self.ln_2(x))

    def decode(self, x, *cache_args):
        x = x + self.attn.decode(self.ln_1(x), *cache_args)
        return x + self.mlp(self.ln_2(x))

    def extend(self, x, *cache_args):
        x = x + self.attn.extend(self.ln_1(x), *cache_args)
        return x + self.mlp(self.ln_2(x))

    def prefill_paged(self, x, *cache_args):
        x = x + self.attn.prefill_paged(self.ln_1(x), *cache_args)
        return x + self.mlp(self.ln_2(x))

    def extend_paged(self, x, *cache_args):
        x = x + self.attn.extend_paged(self.ln_1(x), *cache_args)
        return x + self.mlp(self.ln_2(x))


@dataclass
class KVCache:
    """Per-layer K and V, [B, n_kv_head, max_len, head_dim] each, and the
    number of valid rows of every batch row, int32 [B] on the device. An fp8
    (float8_e4m3fn) cache also carries per-layer fp32 [n_kv_head] scales;
    they stay None for every other dtype."""

    k: List[torch.Tensor]
    v: List[torch.Tensor]
    kv_len: torch.Tensor
    k_scale: Optional[List[torch.Tensor]] = None
    v_scale: Optional[List[torch.Tensor]] = None


@dataclass
class PagedKVCache:
    """Per-layer K and V page pools, [num_pages, n_kv_head, page_size,
    head_dim] each; the number of valid rows of every batch row, int32 [B];
    and the block table, int32 [B, max_pages]: logical row j of batch row b
    is row j % page_size of page block_table[b, j // page_size]. All on the
    device. An fp8 (float8_e4m3fn) cache also carries per-layer fp32
    [n_kv_head] scales; they stay None for every other dtype."""

    k: List[torch.Tensor]
    v: List[torch.Tensor]
    kv_len: torch.Tensor
    block_table: torch.Tensor
    page_size: int
    k_scale: Optional[List[torch.Tensor]] = None
    v_scale: Optional[List[torch.Tensor]] = None


class GPT2(nn.Module):
    def __init__(self, cfg: GPT2Config = None):
        super().__init__()
        cfg = cfg or GPT2Config()
        self.cfg = cfg
        self.wte = nn.Embedding(cfg.vocab_size, cfg.n_embd)
        self.wpe = nn.Embedding(cfg.n_positions, cfg.n_embd)
        self.blocks = nn.ModuleList(Block(cfg) for _ in range(cfg.n_layer))
        self.ln_f = LayerNorm(cfg.n_embd)
        self.lm_head = nn.Linear(cfg.n_embd, cfg.vocab_size, bias=False)
        self.lm_head.weight = self.wte.weight  # tied

        self.apply(self._init_weights)
        # scaled init for residual projections (GPT-2 paper)
        for name, p in self.named_parameters():
            if name.endswith('c_proj.weight') or name.endswith('mlp.2.weight'):
                nn.init.normal_(p, mean=0.0, std=0.02 / math.sqrt(2 * cfg.n_layer))

    @staticmethod
    def _init_weights(module):
        if isinstance(module, nn.Linear):
            nn.init.normal_(module.weight, mean=0.0, std=0.02)
            if module.bias is not None:
                nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            nn.init.normal_(module.weight, mean=0.0, std=0.02)

    def forward(self, idx, targets=None, doc_ids=None):
        B, T = idx.shape
        pos = torch.arange(T, device=idx.device)
        doc_start = None
        if doc_ids is not None:
            # once per step, on the device, no sync; positions restart at
            # each document (a document longer than the table reuses the
            # last position instead of indexing past it)
            doc_start = document_starts(doc_ids)
            pos = (pos - doc_start).clamp(max=self.cfg.n_positions - 1)
        x = self.wte(idx) + self.wpe(pos)
        for block in self.blocks:
            x = block(x, doc_start)
        x = self.ln_f(x)
        logits = self.lm_head(x)
        if targets is None:
            return logits
        # fused online-softmax CE on gfx950 for bf16 logits
        loss = cross_entropy(logits.view(-1, logits.size(-1)), targets.reshape(-1))
        return logits, loss

    def _init_scales(self, dtype, n_kv_head, device):
        # per-layer K and V scales of an fp8 cache, ones; (None, None) otherwise
        if dtype != torch.float8_e4m3fn:
            return None, None
        n_layer = self.cfg.n_layer
        k_scale, v_scale = ([torch.ones(n_kv_head, device=device) for _ in range(n_layer)] for _ in range(2))
        return k_scale, v_scale

    def init_cache(self, batch, max_len, device=None, dtype=None) -> KVCache:
        """An empty cache for `batch` rows of up to `max_len` tokens.
        dtype=torch.float8_e4m3fn makes it an fp8 cache with unit scales."""
        cfg = self.cfg
        device = self.wte.weight.device if device is None else device
        dtype = self.wte.weight.dtype if dtype is None else dtype
        n_kv_head = cfg.n_head if cfg.n_kv_head is None else cfg.n_kv_head
        shape = (batch, n_kv_head, max_len, cfg.n_embd // cfg.n_head)
        k_scale, v_scale = self._init_scales(dtype, n_kv_head, device)
        return KVCache(
            k=[torch.empty(shape, device=device, dtype=dtype) for _ in range(cfg.n_layer)],
            v=[torch.empty(shape, device=device, dtype=dtype) for _ in range(cfg.n_layer)],
            kv_len=torch.zeros(batch, dtype=torch.int32, device=device),
            k_scale=k_scale,
            v_scale=v_scale,
        )

    def init_paged_cache(
        self, batch, max_len, page_size=64, num_pages=None, block_table=None, device=None, dtype=None
    ) -> PagedKVCache:
        """An empty paged cache for `batch` rows of up to `max_len` tokens:
        ceil(max_len / page_size) table entries per row over pools of
        `num_pages` pages (default: one page per entry). The default table
        hands the pages out in order; any integer [batch, max_pages] table
        whose live entries name distinct pages may be passed instead.
        dtype=torch.float8_e4m3fn makes it an fp8 cache with unit scales."""
        cfg = self.cfg
        device = self.wte.weight.device if device is None else device
        dtype = self.wte.weight.dtype if dtype is None else dtype
        n_kv_head = cfg.n_head if cfg.n_kv_head is None else cfg.n_kv_head
        max_pages = -(-max_len // page_size)
        if block_table is None:
            block_table = torch.arange(batch * max_pages, dtype=torch.int32, device=device).view(batch, max_pages)
        else:
            assert block_table.shape == (batch, max_pages), 'block_table must be [batch, ceil(max_len / page_size)]'
            block_table = block_table.to(device=device, dtype=torch.int32).contiguous()
        num_pages = batch * max_pages if num_pages is None else num_pages
        shape = (num_pages, n_kv_head, page_size, cfg.n_embd // cfg.n_head)
        k_scale, v_scale = self._init_scales(dtype, n_kv_head, device)
        return PagedKVCache(
            k=[torch.empty(shape, device=device, dtype=dtype) for _ in range(cfg.n_layer)],
            v=[torch.empty(shape, device=device, dtype=dtype) for _ in range(cfg.n_layer)],
            kv_len=torch.zeros(batch, dtype=torch.int32, device=device),
            block_table=block_table,
            page_size=page_size,
            k_scale=k_scale,
            v_scale=v_scale,
        )

    @torch.no_grad()
    def prefill(self, idx, cache):
        """Run the prompt idx [B, T] through the training attention path,
        fill the cache (either type) with its K/V and return the last
        position's logits [B, vocab]."""
        B, T = idx.shape
        x = self.wte(idx) + self.wpe(torch.arange(T, device=idx.device))
        if self._appends(cache):
            cache.kv_len.fill_(T)
            for block, args in zip(self.blocks, self._append_args(cache)):
                x = block.prefill_paged(x, *args)
            return self.lm_head(self.ln_f(x[:, -1]))
        for block, k_cache, v_cache in zip(self.blocks, cache.k, cache.v):
            x = block.prefill(x, k_cache, v_cache)
        cache.kv_len.fill_(T)
        return self.lm_head(self.ln_f(x[:, -1]))

    @staticmethod
    def _appends(cache):
        """True when the cache is written by `kvcache_append`: paged caches,
        and dense fp8 ones (index writes cannot quantise)."""
        return isinstance(cache, PagedKVCache) or cache.k_scale is not None

    @staticmethod
    def _append_args(cache):
        """Per layer: (k, v, kv_len, block_table or None, k_scale, v_scale)."""
        table = cache.block_table if isinstance(cache, PagedKVCache) else None
        none = [None] * len(cache.k)
        for k, v, ks, vs in zip(cache.k, cache.v, cache.k_scale or none, cache.v_scale or none):
            yield k, v, cache.kv_len, table, ks, vs

    def _extend_paged(self, idx, cache):
        B, T = idx.shape
        rows = cache.kv_len.long().unsqueeze(1) + torch.arange(T, device=idx.device)  # before the increment
        cache.kv_len += T
        x = self.wte(idx) + self.wpe(rows.clamp(max=self.cfg.n_positions - 1))
        for block, args in zip(self.blocks, self._append_args(cache)):
            # (a full cache overwrites its last rows instead of writing past them)
            x = block.extend_paged(x, *args)
        return self.lm_head(self.ln_f(x[:, -1]))

    @torch.no_grad()
    def decode_step(self, tokens, cache):
        """Append one token per row (tokens [B]) to the cache (either type)
        and return the logits [B, vocab] for the token after it. Positions
        come from cache.kv_len on the device; nothing is read back."""
        B = tokens.shape[0]
        if self._appends(cache):
            return self._extend_paged(tokens.view(B, 1), cache)
        pos = cache.kv_len.long()  # the new token's row, before the increment
        cache.kv_len += 1
        batch = torch.arange(B, device=tokens.device)
        x = self.wte(tokens.view(B, 1)) + self.wpe(pos.clamp(max=self.cfg.n_positions - 1)).unsqueeze(1)
        for block, k_cache, v_cache in zip(self.blocks, cache.k, cache.v):
            # (a full cache overwrites its last row instead of writing past it)
            x = block.decode(x, k_cache, v_cache, cache.kv_len, batch, pos.clamp(max=k_cache.shape[2] - 1))
        return self.lm_head(self.ln_f(x[:, 0]))

    @torch.no_grad()
    def extend(self, idx, cache):
        """Append idx [B, T] to a cache (either type) that may already hold
        tokens (each row its own count) and return the last position's logits
        [B, vocab]: chunked prefill, or the next turn of a conversation.
        Positions and cache rows come from cache.kv_len on the device;
        nothing is read back. Attention runs through sdpa_kvcache with
        Nq = T."""
        B, T = idx.shape
        if self._appends(cache):
            return self._extend_paged(idx, cache)
        rows = cache.kv_len.long().unsqueeze(1) + torch.arange(T, device=idx.device)  # [B, T], before the increment
        cache.kv_len += T
        batch = torch.arange(B, device=idx.device).unsqueeze(1)
        x = self.wte(idx) + self.wpe(rows.clamp(max=self.cfg.n_positions - 1))
        for block, k_cache, v_cache in zip(self.blocks, cache.k, cache.v):
            # (a full cache overwrites its last row instead of writing past it)
            x = block.extend(x, k_cache, v_cache, cache.kv_len, batch, rows.clamp(max=k_cache.shape[2] - 1))
        return self.lm_head(self.ln_f(x[:, -1]))

    @torch.no_grad()
    def generate(
        self, idx, max_new_tokens, temperature=0.0, generator=None, prefill_chunk=None, page_size=None, kv_dtype=None
    ):
        """idx [B, T] followed by max_new_tokens sampled tokens,
        [B, T + max_new_tokens]. temperature = 0 is greedy; otherwise the
        next token is drawn from softmax(logits / temperature). The prompt
        runs through `prefill` in one piece, or with prefill_chunk = c >= 1
        through `extend` in pieces of at most c tokens. page_size = p keeps
        the K/V cache in pages of p rows (`init_paged_cache`). kv_dtype is
        the cache's dtype (None: the weights'; torch.float8_e4m3fn: an fp8
        cache with unit scales)."""
        B, T = idx.shape
        assert T >= 1 and T + max_new_tokens <= self.cfg.n_positions, 'sequence exceeds n_positions'
        if page_size is None:
            cache = self.init_cache(B, T + max_new_tokens, dtype=kv_dtype)
        else:
            cache = self.init_paged_cache(B, T + max_new_tokens, page_size, dtype=kv_dtype)
        out = [idx]
        if prefill_chunk is None:
            logits = self.prefill(idx, cache)
        else:
            assert prefill_chunk >= 1, 'prefill_chunk must be >= 1'
            for piece in idx.split(prefill_chunk, dim=1):
                logits = self.extend(piece, cache)
        for step in range(max_new_tokens):
            if step > 0:
                logits = self.decode_step(out[-1].view(B), cache)
            if temperature == 0.0:
                nxt = logits.argmax(dim=-1, keepdim=True)
            else:
                probs = torch.softmax(logits.float() / temperature, dim=-1)
                nxt = torch.multinomial(probs, 1, generator=generator)
            out.append(nxt)
        return torch.cat(out, dim=1)


def gpt2_small(n_kv_head: Optional[int] = None) -> GPT2:
    return GPT2(GPT2Config(n_kv_head=n_kv_head))


def gpt2_tiny(n_kv_head: Optional[int] = None) -> GPT2:
    """Small config for CPU tests."""
    return GPT2(GPT2Config(vocab_size=512, n_positions=64, n_embd=64, n_layer=2, n_head=2, n_kv_head=n_kv_head))
