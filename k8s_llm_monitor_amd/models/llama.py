"""Decoder-only causal LMs served by the diagnostic engine: Llama-3 and Qwen3 (dense), Mixtral (MoE)
and GPT-2 (the CPU plumbing config), with Megatron tensor parallelism.

Nothing here exists in the reference ("no LLM, no GPU code"); the model replaces
the remote ``callLLMAPI`` step of the doc sketch ``docs/metrics-usage-example.md:244-306``.

Prefill layer (GPU, TP=1), every GEMM on the hand-written 256 x 256 MFMA tile kernel
(ops/csrc/gemm_tile.hip) with its epilogue doing the elementwise work - fragment-packed weights go
there at any row count, row-major ones from ops.TILE_MIN_M rows, and from that many rows the
RMSNorms live in the epilogues as well (``_prefill_fused_norm``):

  qkv (+ RoPE of q / k, rows scaled by 1/rms) -> rope_and_cache (paged KV write) -> flash_prefill
  -> o (+ residual add, next norm's operand and sums of squares) -> gate_up (+ SwiGLU, row scale)
  -> down (+ residual add, ...)

TP > 1 prefill runs as two micro-batches whose row-parallel all-reduces overlap each other's
compute (``_prefill_overlap``).

Decode layer (``_decode_layers_skinny``, 7 launches inside one hipGraph): qkv (split-K slabs) ->
paged_decode_fused (slab reduce + RoPE + KV write + attention) -> o (slabs) -> add_norm_partial
(residual add, deferred norm) -> gate_up + SwiGLU -> down (slabs) -> add_norm_partial.  The
projections and the LM head run on the shared-A decode GEMM over fragment-packed weights
(ops/csrc/gemm_decode.hip), or on the row-major skinny kernel (gemm_skinny.hip) where no packed
form exists.

Qwen3 (``cfg.qk_norm``: a learned RMSNorm over head_dim on every q and k head, before RoPE) takes
the norm inside rope_and_cache's kernel, so neither the qkv GEMM's RoPE epilogue nor the fused
decode attention applies.  Prefill: qkv (plain) -> rope_and_cache (QK-norm + RoPE + KV write) ->
flash_prefill, the RMSNorms between projections as fused_add_rms_norm launches.  Decode (8
launches): qkv (slabs) -> rope_and_cache (slab reduce + QK-norm + RoPE + KV write) -> paged_decode
-> o ... as above.  ``q_norm`` / ``k_norm`` ([D]) are whole on every TP rank.

Weights are stored fused and pre-sharded: ``wqkv`` [(Hq+2Hkv)/tp * D, d] (column-parallel),
``wo`` [d, Hq/tp * D] (row-parallel), ``w13`` [2F/tp, d] (this rank's gate and up rows), ``w2``
[d, F/tp].  Random init is seeded per tensor name, and every rank generates the full tensor then
keeps its shard, so any TP degree reproduces the TP=1 model exactly.

The four projections of every layer are resident in ONE of three layouts (``CausalLM._layout``):

  CANONICAL    row-major [out, in], w13 as [gate; up] - the checkpoint's form (GPT-2; F no multiple of 64)
  INTERLEAVED  row-major, w13 interleaved per 128 rows as [64 gate | 64 up] (the SwiGLU
               epilogues' pairing); decode reads views (``*_p`` / ``*_pg``) or packed copies
               (``*_d`` / ``*_dg``) next to it
  PACKED       ``ONE_LAYOUT``: the fragment-packed tensor [out/16, in/32, 64, 8] is the only copy
               (w13 paired per 16 rows as [8 gate | 8 up]); prefill's tile GEMM reads it too and
               ``*_d`` / ``*_dg`` are the weights themselves

With ``PREFILL_WEIGHTS = "fp8"`` a PACKED dense projection may be resident as its fp8 encoding
ONLY: ``L[key]`` is then the packed e4m3 codes ([out/16, in/64, 64, 16], also under ``*_q``) with
the row scales under ``*_qs`` and no ``*_d`` - prefill's tile GEMM and the decode GEMMs both read
the codes (``_release_bf16``).  ``PREFILL_WEIGHTS = "mxfp4"`` does the same over the mxfp4 encoding:
``L[key]`` is the packed e2m1 codes ([out/16, in/128, 64, 16] uint8) and ``*_qs`` their packed e8m0
block scales; ``ops.is_codes`` is true of either.

Per-request LoRA adapters (``enable_lora`` / ``load_adapter``, ``AttnMeta.lora_slot``): one base model
stays resident and a step's rows may each name an adapter of the arena (ops.LoraState).  On the skinny
decode loop an adapter's delta is one more split-K slab after the qkv, o and down GEMMs (ops.lora_slab;
their consumers sum ``ns + 1`` slabs); the generic layer loop adds it in place (ops.lora_add) to the
plain qkv (before the rotation), o and dense down outputs.  The gate_up delta (``enable_lora(mlp=True)``,
arena "w13" in the resident w13's row order) enters before SwiGLU: the decode gate_up GEMM adds it to
its accumulator (ops.dec_gemm ``delta``, over the PACKED w13), the generic layer loop runs gate_up
plain, adds it and pairs gate and up in ops.silu_mul.  A step without ``lora_slot`` takes exactly
the paths it takes without adapters.

``to_resident`` / ``to_canonical`` convert one projection between CANONICAL and another layout;
``_init_skinny`` / ``_init_dec`` move a model forward, ``begin_load`` takes it out of service
(LOADING) until the loader's closing ``_init_skinny``.
"""
from __future__ import annotations

import hashlib
import logging
import math
import os
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from .. import ops
from ..ops import reference as ref
from ..parallel.comm import (kv_head_range, shard_range, tp_all_gather_last, tp_all_gather_rows, tp_all_reduce,
                             tp_all_reduce_async, tp_all_to_all)
from ..parallel.state import ParallelState, get_state
from .config import ModelConfig

log = logging.getLogger(__name__)

@dataclass
class AttnMeta:
    """Per-step batch metadata (built by the engine's model runner)."""

    is_prefill: bool
    positions: torch.Tensor  # [T] int32
    slot_mapping: torch.Tensor  # [T] int32, -1 = do not write the cache
    # prefill (whole prompts in this step)
    cu_seqlens: Optional[torch.Tensor] = None  # [S+1] int32
    qb_seq: Optional[torch.Tensor] = None  # flash_prefill q-block schedule
    qb_start: Optional[torch.Tensor] = None
    logits_idx: Optional[torch.Tensor] = None  # [S] int64 rows that produce logits
    ctx_start: Optional[torch.Tensor] = None  # [S] int32 cached prefix tokens (paged prefill) or None
    # decode (one token per sequence)
    block_tables: Optional[torch.Tensor] = None  # [B, W] int32
    seq_lens: Optional[torch.Tensor] = None  # [B] int32 (including the token being decoded)
    decode_ws: Optional[tuple] = None  # paged_decode partial buffers
    # mixed prefill+decode step (is_prefill): the first num_decode rows are single decode tokens
    # attending their paged context through paged_decode; cu_seqlens / qb_* / ctx_start /
    # block_tables then describe the prefill rows that follow
    num_decode: int = 0
    dec_block_tables: Optional[torch.Tensor] = None  # [num_decode, W] int32
    dec_seq_lens: Optional[torch.Tensor] = None  # [num_decode] int32 (including the decoded token)
    # pipelined decode inputs: row i feeds dec_prev[dec_src[i]] when dec_src[i] >= 0 (the token the
    # previous step sampled, still on the device), else ids[i]; resolved inside the first kernel
    dec_src: Optional[torch.Tensor] = None  # [B] int32
    dec_prev: Optional[torch.Tensor] = None  # [>= B] int32
    # TP > 1 prefill as two micro-batches of whole sequences: (meta of rows [0, TA), meta of rows
    # [TA, T), TA); their row-parallel all-reduces overlap each other's compute (_prefill_overlap)
    micro: Optional[tuple] = None
    # per-request LoRA: the adapter slot of every row of the step ([T] int32, -1 = the base model);
    # None when no row uses an adapter - the step then takes exactly the paths it takes without LoRA
    lora_slot: Optional[torch.Tensor] = None
    # embedding requests (prefill steps only): pool_dim [R] int32 aligned with logits_idx, > 0 = the
    # row is an embedding row of that many dimensions; forward leaves ops.pool_l2's fp32 [R, d_model]
    # in ``pooled``.  None = no embedding row.  want_logits False: no row of the step needs a token,
    # the LM head is not run and forward returns an empty [0, vocab] tensor
    pool_dim: Optional[torch.Tensor] = None
    want_logits: bool = True
    pooled: Optional[torch.Tensor] = None


def _seed_for(name: str, seed: int) -> int:
    h = hashlib.blake2b(f"{seed}:{name}".encode(), digest_size=8).digest()
    return int.from_bytes(h, "little") & 0x7FFF_FFFF_FFFF_FFFF


# CausalLM._layout: the resident layout of the projections (module docstring); LOADING = no usable
# weights, between begin_load() and the _init_skinny() that closes a load
CANONICAL, INTERLEAVED, PACKED, LOADING = "canonical", "interleaved", "packed", "loading"
PROJ = ("wqkv", "wo", "w13", "w2")
# layer-dict keys with these suffixes are derived from the projections, not parameters: the
# gemm_skinny views (dense, expert stack), the decode GEMM's packed copies (dense, expert stack)
# and, with DEC_WEIGHTS = "fp8", the fp8 encoding of a dense projection (packed e4m3 codes, per-row scales;
# with PREFILL_WEIGHTS = "fp8" / "mxfp4" the codes may be the projection itself: L[key] is L[key + "_q"], no "_d")
# or, with DEC_WEIGHTS = "mxfp4", its mxfp4 encoding under the same two keys (ops.pack_skinny_f4's
# codes and block scales; ops.is_mxfp4 / ops.is_fp8 tell the two apart)
# (MoE expert stacks: the same two keys hold 5-d [E, ...] stacks of per-expert codes and scales)
DERIVED = ("_p", "_pg", "_d", "_dg", "_q", "_qs")
DEC_COPIES = ("_d", "_dg")  # the decode GEMM's packed bf16 copies among them


def _each(w: torch.Tensor, fn) -> torch.Tensor:
    """``fn`` of a dense weight, or of every expert of an [E, ...] stack (row-major or packed)."""
    return torch.stack([fn(e) for e in w]) if w.dim() in (3, 5) else fn(w)


def to_resident(w: torch.Tensor, key: str, form: str) -> torch.Tensor:
    """Projection ``key`` (or its expert stack) from CANONICAL to the layout ``form``."""
    if form == PACKED:
        return _each(w, lambda e: ops.pack_skinny(ops.interleave_gate_up8(e) if key == "w13" else e))
    return _each(w, ops.interleave_gate_up) if key == "w13" and form == INTERLEAVED else w


def to_canonical(w: torch.Tensor, key: str, form: str, scale: Optional[torch.Tensor] = None,
                 dtype=torch.bfloat16) -> torch.Tensor:
    """Projection ``key`` (or its expert stack) resident as ``form``, back to CANONICAL.  A
    projection resident as its fp8 or mxfp4 encoding only (packed codes, ``scale`` its row scales in
    packed row order / its packed block scales) is dequantised to ``dtype`` - exactly the bf16
    values it was quantised from."""
    if ops.is_codes(w):
        d = ops.dequantize_codes(w, scale, dtype)
        return ops.deinterleave_gate_up8(d) if key == "w13" else d
    if form == PACKED:
        return _each(w, lambda e: ops.deinterleave_gate_up8(ops.unpack_skinny(e)) if key == "w13"
                     else ops.unpack_skinny(e))
    return _each(w, ops.deinterleave_gate_up) if key == "w13" and form == INTERLEAVED else w


def relayout(w: torch.Tensor, key: str, src: str, dst: str) -> torch.Tensor:
    """``src`` -> CANONICAL -> ``dst``, expert by expert (one expert's intermediates at a time);
    ``w`` itself where the two layouts store this projection alike."""
    if key != "w13":  # only w13 tells INTERLEAVED from CANONICAL
        src, dst = (f if f == PACKED else CANONICAL for f in (src, dst))
    return w if src == dst else _each(w, lambda e: to_resident(to_canonical(e, key, src), key, dst))


class CausalLM:
    # path selection for tests and tools (class attributes, not environment switches):
    # SKINNY_DECODE False = decode through the plain row-major path (the fp32-reference form of the
    # real-shape tests); DECODE_GEMM "auto" | "dec" | "rm" = the decode projections' kernel (_want_dec)
    SKINNY_DECODE = True
    DECODE_GEMM = "auto"
    # ONE resident copy of every dense Llama projection on the GPU: the decode GEMMs' fragment-packed
    # layout, which the prefill tile GEMM reads as well (gemm_tile wpk mode - bit-identical to the
    # row-major form and within +-1.4 % of its speed: profiles/r06/gemm_packed_w_*.jsonl); the
    # row-major tensors are dropped.  "force": also on the CPU (tests).
    ONE_LAYOUT = True
    # The encoding the decode GEMMs stream the dense projections and the LM head from: "bf16", or
    # "fp8" - per weight row e4m3 codes times a power-of-two scale (ops.quantize_rows_fp8).  The
    # model's bf16 weights then ARE the dequantised values (one model, two encodings: prefill, the
    # row-complete o projection, the TP tails, canonical() / save_checkpoint and the fp32 reference
    # read them unchanged) and the fp8 copy sits beside them (resident weights grow by half; only
    # decode gets faster).  Per launch the fp8 encoding is used where gemm_decode.hip has an fp8
    # form for the shape and row count (ops.dec_config(f8=True)), the bf16 copy otherwise.
    # "mxfp4" - the same two-copy design over OCP MXFP4 (ops.quantize_mxfp4: e2m1 codes with one
    # e8m0 scale per 32 elements along K): the bf16 weights are the dequantised values, the codes
    # and block scales sit beside them under the same ``*_q`` / ``*_qs`` keys (resident weights
    # grow by 17/64), and a launch streams them where ops.dec_config(f4=True) has a form.
    # MoE expert stacks are quantised under either encoding too (5-d ``w13_q`` / ``w2_q`` stacks
    # beside the bf16 stacks, _quantize_experts) and the grouped launches of up to 64 rows stream
    # them (ops.dec_grouped_q_config, _dec_grouped); prefill and the routed > 64-row decode path
    # read the bf16 stacks, which hold the dequantised values.
    DEC_WEIGHTS = "bf16"
    # What prefill reads where DEC_WEIGHTS = "fp8": "bf16" - the bf16 copy beside the codes - or
    # "fp8": the tile GEMM converts the codes on the way into the MFMA (gemm_tile.hip F8,
    # bit-identical) and the bf16 copy of every dense projection (and the head) whose decode
    # launches all have an fp8 form is released: the codes are the only resident copy
    # (_f8_only_ok; dense, TP = 1, ONE_LAYOUT models - every other projection keeps both copies).
    # "mxfp4", where DEC_WEIGHTS = "mxfp4": the same over the mxfp4 codes and block scales
    # (gemm_tile.hip F4) - prefill and decode read one tensor, a quarter of the bf16 bytes.
    PREFILL_WEIGHTS = "bf16"
    # The last layer of a dense TP = 1 prefill runs o, gate_up and down on the rows of
    # ``meta.logits_idx`` only (its qkv, KV write and attention still see every row): the layers
    # above need every row of the residual stream, the final norm and the head only those.  Every
    # GEMM of that tail is one whose rows do not depend on each other (the tile kernel, or the CPU
    # reference), so the logits are bit-identical to the full-row form's.  False: the full-row form (A/B).
    LAST_LAYER_ROWS = True
    # False after load_checkpoint read a checkpoint with neither an lm_head nor tied embeddings (the
    # base-model save form embedding models ship as): lm_head is then the embedding matrix standing
    # in, and the engine refuses generation requests
    has_head = True

    def __init__(self, cfg: ModelConfig, device: torch.device | str = "cpu", dtype=torch.bfloat16, seed: int = 0,
                 pstate: Optional[ParallelState] = None, init_std: float = 0.02, init: str = "random",
                 dec_weights: Optional[str] = None, prefill_weights: Optional[str] = None):
        """``init``: "random" (seeded per tensor name) or "empty" (uninitialised storage, for
        models about to be filled by models/checkpoint.load_checkpoint).  ``dec_weights``: this
        model's DEC_WEIGHTS ("bf16" | "fp8" | "mxfp4"; None = the class constant); ``prefill_weights``: its
        PREFILL_WEIGHTS ("bf16" | "fp8" | "mxfp4", a quantised one only on top of the same decode weights)."""
        if init not in ("random", "empty"):
            raise ValueError(f"init must be 'random' or 'empty', not {init!r}")
        if dec_weights is not None:
            self.DEC_WEIGHTS = dec_weights
        if self.DEC_WEIGHTS not in ("bf16", "fp8", "mxfp4"):
            raise ValueError(f"decode weights must be 'bf16', 'fp8' or 'mxfp4', not {self.DEC_WEIGHTS!r}")
        if prefill_weights is not None:
            self.PREFILL_WEIGHTS = prefill_weights
        if self.PREFILL_WEIGHTS not in ("bf16", "fp8", "mxfp4"):
            raise ValueError(f"prefill weights must be 'bf16', 'fp8' or 'mxfp4', not {self.PREFILL_WEIGHTS!r}")
        if self.PREFILL_WEIGHTS != "bf16" and self.DEC_WEIGHTS != self.PREFILL_WEIGHTS:
            raise ValueError(f"prefill weights {self.PREFILL_WEIGHTS!r} need decode weights {self.PREFILL_WEIGHTS!r} "
                             "(the codes prefill reads are decode's)")
        self._empty_init = init == "empty"
        self._f8_defer = self._empty_init  # uninitialised storage is not quantised: the load's closing _init_skinny does
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype
        self.seed = seed
        self.ps = pstate or get_state()
        tp, r = self.ps.tp_size, self.ps.tp_rank
        kv_ok = cfg.n_kv_heads % tp == 0 or tp % cfg.n_kv_heads == 0  # shard, or replicate (kv_head_range)
        if cfg.n_heads % tp or not kv_ok or cfg.ffn_dim % tp or cfg.vocab_size_padded(tp) % tp:
            raise ValueError(f"{cfg.name}: heads/ffn/vocab not divisible by tp={tp}")
        self.tp, self.rank = tp, r
        self.hq = cfg.n_heads // tp
        self.hkv = max(1, cfg.n_kv_heads // tp)
        self.D = cfg.head_dim
        self.f_local = cfg.ffn_dim // tp
        self.vocab_padded = cfg.vocab_size_padded(tp)
        self.v_lo, self.v_hi = shard_range(self.vocab_padded, tp, r)
        self.scale = 1.0 / math.sqrt(self.D)
        self.std = init_std
        if cfg.is_moe:
            if cfg.n_experts % tp:
                raise ValueError("n_experts must be divisible by tp for expert parallelism")
            self.e_lo, self.e_hi = shard_range(cfg.n_experts, tp, r)
        self.moe_comm = os.environ.get("K8SLLM_MOE_COMM", "a2a")  # "a2a" (prefill all-to-all EP) | "allreduce"
        # MoE prefill GEMMs: "grouped" (default) = one launch per projection over all local
        # experts from the device-side offsets (gemm_tile.hip 256 x 256 tiles, SwiGLU fused; zero
        # host syncs, capturable); "loop" = one hipBLASLt GEMM per expert after a host sync of the
        # expert offsets.  Mixtral-8x7B end to end: 8.14 vs 8.11 q/s (profiles/r02)
        self._moe_grouped = True
        # MoE decode at TP>1: "allreduce" = every rank runs its experts on every (replicated)
        # token, dense-masked, then one all-reduce; "a2a" = expert-parallel dispatch / combine with
        # static-capacity all-to-alls (_moe_a2a_decode, graph-capturable)
        self.moe_decode = os.environ.get("K8SLLM_MOE_DECODE", "allreduce")
        self.layers: list[dict] = []
        self._layout = CANONICAL  # what _build makes; assigned by _init_skinny / _init_dec / begin_load only
        self.skinny_layout = None
        # the decode path's state, (re)built by _init_skinny
        self._skinny_ws = self.lm_head_d = self.lm_head_q = self.lm_head_qs = None
        self._rc_o, self._dec_wide, self._attn_rope = 0, False, False
        self.lora: Optional[ops.LoraState] = None  # the resident adapters' arena (enable_lora)
        self._lora_cap = 0
        self._lora_w13_layout = CANONICAL  # the row order of the gate_up arena's B (enable_lora(mlp=True))
        self._build()
        self._init_skinny()
        self.cos_sin = None
        if cfg.arch == "llama":
            self.cos_sin = ref.rope_cos_sin(cfg.max_position, self.D, cfg.rope_theta, cfg.rope_scaling,
                                            device=self.device)

    # ------------------------------------------------------------------ weights
    # what the kernels' callers ask of the layout (read-only: _layout is the state)
    @property
    def _w13_il(self) -> bool:
        """w13's gate / up rows are interleaved: per 128 rows, or per 16 inside the packed form,
        which the per-expert fallback paths unpack to the per-128 pairing (_expert)."""
        return self._layout in (INTERLEAVED, PACKED)

    @property
    def _packed(self) -> bool:
        """ONE_LAYOUT: the projections are resident fragment-packed only."""
        return self._layout == PACKED

    @property
    def _swg(self):
        """gemm_tile's SwiGLU pairing of w13: True = per 128 rows, 8 = per 16 (packed)."""
        return 8 if self._layout == PACKED else True

    @staticmethod
    def _drop_derived(L: dict, every: bool = False) -> None:
        """Drop the layer's derived tensors - but, unless ``every``, not the codes and scales of a
        projection that is resident as its fp8 encoding only: those ARE the weight (``_remat``
        turns it back)."""
        keep = set() if every else {key + sfx for key in PROJ if ops.is_codes(L.get(key)) for sfx in ("_q", "_qs")}
        for k in [k for k in L if k.endswith(DERIVED) and k not in keep]:
            del L[k]

    @staticmethod
    def _wsc(L: dict, key: str) -> Optional[torch.Tensor]:
        """The scales the tile GEMM needs with ``L[key]``: those of a codes-only projection."""
        return L[key + "_qs"] if ops.is_codes(L[key]) else None

    def begin_load(self) -> None:
        """Before a loader replaces the weights: the derived tensors (decode copies; under
        ONE_LAYOUT aliases of the packed weights) go first, so that peak memory stays about one
        copy of the model (Llama-3-70B at TP=1 would not fit two), and the model is out of service
        (LOADING: forward raises) until the loader's closing ``_init_skinny``, which takes the
        projections it finds for CANONICAL."""
        self.lm_head_d = self.lm_head_q = self.lm_head_qs = None
        self._f8_defer = False
        for L in self.layers:
            self._drop_derived(L, every=True)  # the loader replaces every projection, fp8-only ones too
        self._layout = LOADING

    def _rand(self, name: str, shape, std: Optional[float] = None) -> torch.Tensor:
        if self._empty_init:
            return torch.empty(shape, dtype=self.dtype, device=self.device)
        g = torch.Generator(device=self.device)
        g.manual_seed(_seed_for(name, self.seed))
        t = torch.empty(shape, dtype=torch.float32 if self.device.type == "cpu" else self.dtype, device=self.device)
        t.normal_(0.0, self.std if std is None else std, generator=g)
        return t.to(self.dtype)

    def _ones(self, n) -> torch.Tensor:
        return torch.ones(n, dtype=self.dtype, device=self.device)

    def _zeros(self, n) -> torch.Tensor:
        return torch.zeros(n, dtype=self.dtype, device=self.device)

    def _build(self) -> None:
        c = self.cfg
        d, D, tp, r = c.d_model, self.D, self.tp, self.rank
        out_std = self.std / math.sqrt(2 * c.n_layers)
        emb = self._rand("embed", (self.vocab_padded, d))
        self.embed = emb[self.v_lo:self.v_hi].contiguous()
        del emb
        if c.tie_embeddings:
            self.lm_head = self.embed
        else:
            lm = self._rand("lm_head", (self.vocab_padded, d))
            self.lm_head = lm[self.v_lo:self.v_hi].contiguous()
            del lm
        if c.arch == "gpt2":
            self.pos_embed = self._rand("pos_embed", (c.max_position, d), 0.01)
            self.final_norm = (self._ones(d), self._zeros(d))
        else:
            self.final_norm = self._ones(d)
        q_lo, q_hi = shard_range(c.n_heads * D, tp, r)
        kv_lo, kv_hi = kv_head_range(c.n_kv_heads, D, tp, r)
        f_lo, f_hi = shard_range(c.ffn_dim, tp, r)
        for i in range(c.n_layers):
            p = f"layers.{i}."
            L: dict = {}
            wq = self._rand(p + "wq", (c.n_heads * D, d))
            wk = self._rand(p + "wk", (c.n_kv_heads * D, d))
            wv = self._rand(p + "wv", (c.n_kv_heads * D, d))
            L["wqkv"] = torch.cat([wq[q_lo:q_hi], wk[kv_lo:kv_hi], wv[kv_lo:kv_hi]], 0).contiguous()
            del wq, wk, wv
            wo = self._rand(p + "wo", (d, c.n_heads * D), out_std)
            L["wo"] = wo[:, q_lo:q_hi].contiguous()
            del wo
            if c.arch == "gpt2":
                L["ln1"] = (self._ones(d), self._zeros(d))
                L["ln2"] = (self._ones(d), self._zeros(d))
                bqkv = self._rand(p + "bqkv", ((c.n_heads + 2 * c.n_kv_heads) * D,), 0.01)
                nq, nk = c.n_heads * D, c.n_kv_heads * D
                L["bqkv"] = torch.cat([bqkv[q_lo:q_hi], bqkv[nq + kv_lo:nq + kv_hi],
                                       bqkv[nq + nk + kv_lo:nq + nk + kv_hi]]).contiguous()
                L["bo"] = self._rand(p + "bo", (d,), 0.01)  # added once (rank 0 adds it before the reduce)
                w1 = self._rand(p + "w1", (c.ffn_dim, d))
                L["w1"] = w1[f_lo:f_hi].contiguous()
                L["b1"] = self._rand(p + "b1", (c.ffn_dim,), 0.01)[f_lo:f_hi].contiguous()
                w2 = self._rand(p + "w2", (d, c.ffn_dim), out_std)
                L["w2"] = w2[:, f_lo:f_hi].contiguous()
                L["b2"] = self._rand(p + "b2", (d,), 0.01)
                del w1, w2
            else:
                L["attn_norm"] = self._ones(d)
                L["mlp_norm"] = self._ones(d)
                if c.qk_norm:  # one [D] weight for all q heads, one for all k heads: whole on every rank
                    L["q_norm"] = (1.0 + self._rand(p + "q_norm", (D,), 0.1).float()).to(self.dtype)
                    L["k_norm"] = (1.0 + self._rand(p + "k_norm", (D,), 0.1).float()).to(self.dtype)
                if c.is_moe:
                    L["router"] = self._rand(p + "router", (c.n_experts, d))
                    w13, w2s = [], []
                    for e in range(self.e_lo, self.e_hi):
                        g = self._rand(p + f"experts.{e}.w1", (c.ffn_dim, d))
                        u = self._rand(p + f"experts.{e}.w3", (c.ffn_dim, d))
                        w13.append(torch.cat([g, u], 0))
                        w2s.append(self._rand(p + f"experts.{e}.w2", (d, c.ffn_dim), out_std))
                        del g, u
                    L["w13"] = torch.stack(w13).contiguous()  # [E_local, 2F, d]
                    L["w2"] = torch.stack(w2s).contiguous()  # [E_local, d, F]
                    del w13, w2s
                else:
                    g = self._rand(p + "w1", (c.ffn_dim, d))
                    u = self._rand(p + "w3", (c.ffn_dim, d))
                    L["w13"] = torch.cat([g[f_lo:f_hi], u[f_lo:f_hi]], 0).contiguous()
                    del g, u
                    w2 = self._rand(p + "w2", (d, c.ffn_dim), out_std)
                    L["w2"] = w2[:, f_lo:f_hi].contiguous()
                    del w2
            self.layers.append(L)

    # ------------------------------------------------------------------ per-request LoRA adapters
    # PEFT target module -> (adapted projection, its block inside the fused qkv)
    LORA_MODULES = {"q_proj": ("wqkv", 0), "k_proj": ("wqkv", 1), "v_proj": ("wqkv", 2), "o_proj": ("wo", 0),
                    "down_proj": ("w2", 0), "gate_proj": ("w13", 0), "up_proj": ("w13", 1)}

    def enable_lora(self, slots: int, max_rank: int = 64, mlp: bool = False) -> "ops.LoraState":
        """Allocate the adapters' arena (ops.LoraState, ``slots`` adapters of rank up to
        ``max_rank``) and one more slab per projection in the decode workspace.  The fused qkv is
        one adapted projection of rank capacity 3 x the rounded ``max_rank``: q, k and v at their own
        rank rows, B block-diagonal over their output ranges.  ``mlp``: also the fused gate_up
        ("w13", rank capacity 2 x: gate and up at their own rank rows, B block-diagonal, its rows in
        the row order of the resident w13) - opt-in because it about doubles the arena (B is
        [2 F, 2 cap] per layer and slot); without it adapters on gate_proj / up_proj are refused.
        Steps name their rows' adapters through ``AttnMeta.lora_slot``; without it nothing changes."""
        c = self.cfg
        if mlp and c.is_moe:
            raise ValueError("LoRA adapters on gate_proj / up_proj (mlp=True) are not supported on a MoE model")
        if self.tp > 1:
            raise ValueError("LoRA adapters need tp_size == 1 (the TP workers replay the leader's staging words, "
                             "which carry no adapter slots)")
        if c.arch == "gpt2":
            raise ValueError("LoRA adapters are not supported for arch 'gpt2' (Llama-family models only)")
        if max_rank < 1:
            raise ValueError(f"lora_max_rank must be >= 1, not {max_rank}")
        cap = -(-int(max_rank) // ops.LORA_RANK_ALIGN) * ops.LORA_RANK_ALIGN
        d, no = c.d_model, self.hq * self.D
        dims = {"wqkv": ((self.hq + 2 * self.hkv) * self.D, d, 3 * cap), "wo": (d, no, cap)}
        if not c.is_moe:
            dims["w2"] = (d, self.f_local, cap)
        if mlp:
            dims["w13"] = (2 * self.f_local, d, 2 * cap)
        self.lora = ops.LoraState(slots, c.n_layers, dims, self.device, self.dtype)
        self._lora_cap, self._lora_max_rank = cap, int(max_rank)
        self._lora_w13_layout = CANONICAL if self._layout == LOADING else self._layout  # the row order of B["w13"]
        if self._skinny_ws is not None:
            self._skinny_ws = torch.empty(self._skinny_ws_numel(), dtype=torch.float32, device=self.device)
        return self.lora

    def load_adapter(self, slot: int, adapter) -> None:
        """Make arena slot ``slot`` the adapter (models/checkpoint.py ``LoraAdapter``): every
        ``(layer, module)`` pair into its projection, zeros where the adapter has no target.  Raises
        ValueError, naming the reason, for what the serving path cannot apply."""
        if self.lora is None:
            raise ValueError("load_adapter: no LoRA arena (enable_lora first)")
        c, name = self.cfg, getattr(adapter, "name", "") or "adapter"
        for t in adapter.target_modules:
            if t in ("gate_proj", "up_proj") and "w13" not in self.lora.dims:
                raise ValueError(f"LoRA {name}: target module {t!r} is not supported by this arena (the decode gate_up "
                                 "GEMM fuses SwiGLU into its epilogue, so the delta enters before it through an arena "
                                 "of its own: enable_lora(.., mlp=True))")
            if t not in self.LORA_MODULES:
                raise ValueError(f"LoRA {name}: unknown target module {t!r}")
            if t == "down_proj" and c.is_moe:
                raise ValueError(f"LoRA {name}: target module 'down_proj' is not supported on a MoE model")
        if adapter.r > self._lora_max_rank:
            raise ValueError(f"LoRA {name}: rank {adapter.r} exceeds lora_max_rank {self._lora_max_rank}")
        d, D = c.d_model, self.D
        shapes = {"q_proj": (self.hq * D, d), "k_proj": (self.hkv * D, d), "v_proj": (self.hkv * D, d),
                  "o_proj": (d, self.hq * D), "down_proj": (d, self.f_local),
                  "gate_proj": (self.f_local, d), "up_proj": (self.f_local, d)}
        n0 = {0: 0, 1: self.hq * D, 2: (self.hq + self.hkv) * D}
        for (layer, mod), (A, B) in adapter.tensors.items():
            if mod not in adapter.target_modules:
                raise ValueError(f"LoRA {name}: tensors for {mod!r}, which is not among its target modules")
            if not 0 <= layer < c.n_layers:
                raise ValueError(f"LoRA {name}: layer {layer} outside the base model's {c.n_layers} layers")
            out, inn = shapes[mod]
            if tuple(A.shape) != (adapter.r, inn) or tuple(B.shape) != (out, adapter.r):
                raise ValueError(f"LoRA {name}: layer {layer} {mod} lora_A {list(A.shape)} / lora_B {list(B.shape)} do "
                                 f"not match the base model's [{out}, {inn}] at rank {adapter.r}")
        for p in self.lora.dims:  # a reload of the slot leaves nothing of the adapter before
            self.lora.A[p][:, slot].zero_()
            self.lora.B[p][:, slot].zero_()
        rows13 = None
        for (layer, mod), (A, B) in adapter.tensors.items():
            proj, blk = self.LORA_MODULES[mod]
            if proj == "w13":
                # gate / up rows [0, F) / [F, 2F) of the canonical w13, scattered to where the
                # resident layout keeps them
                if rows13 is None:
                    rows13 = self._w13_row_order(self._lora_w13_layout).argsort()
                dst = rows13[blk * self.f_local:(blk + 1) * self.f_local]
                r0 = blk * self._lora_cap
                self.lora.A[proj][layer, slot, r0:r0 + adapter.r] = A.to(self.device, self.dtype)
                self.lora.B[proj][layer, slot, dst.to(self.device), r0:r0 + adapter.r] = B.to(self.device, self.dtype)
                continue
            self.lora.load(slot, layer, proj, A, B, r0=blk * self._lora_cap, n0=n0[blk] if proj == "wqkv" else 0)
        self.lora.set_scaling(slot, adapter.scaling)

    def _w13_row_order(self, layout: str) -> torch.Tensor:
        """``order[n]`` = the canonical ([gate; up]) row of w13 that ``layout`` keeps at row ``n``."""
        idx = torch.arange(2 * self.f_local).view(-1, 1)
        if layout == PACKED:
            idx = ops.interleave_gate_up8(idx)
        elif layout == INTERLEAVED:
            idx = ops.interleave_gate_up(idx)
        return idx.flatten()

    def _lora_relayout(self) -> None:
        """After the resident layout changed (_init_skinny / _init_dec): the rows of the w13 arena's
        B follow the resident w13's new row order, so a loaded adapter never meets a stale pairing."""
        if self.lora is None or "w13" not in self.lora.dims or self._layout == LOADING:
            return
        old, new = self._lora_w13_layout, self._layout
        if old == new:
            return
        # resident_new[n] = canonical[order_new[n]] = resident_old[inverse(order_old)[order_new[n]]]
        src = self._w13_row_order(old).argsort()[self._w13_row_order(new)].to(self.device)
        B = self.lora.B["w13"]
        for layer in range(B.shape[0]):  # one layer's copy at a time
            B[layer] = B[layer].index_select(1, src)
        self._lora_w13_layout = new

    def resident_weight_bytes(self) -> int:
        """Bytes of every distinct weight tensor this rank holds (parameters, decode-layout copies,
        the LM head's packed copy and the fp8 / mxfp4 encodings with their scales; a tensor referenced
        under two keys counts once - the codes of a codes-only projection are its parameter)."""
        seen, n = set(), 0
        ts = [self.embed, self.lm_head, self.lm_head_d, self.lm_head_q, self.lm_head_qs, self.final_norm]
        for L in self.layers:
            for v in L.values():
                ts.extend(v if isinstance(v, tuple) else (v,))
        for t in ts:
            if isinstance(t, torch.Tensor) and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                n += t.numel() * t.element_size()
        return n

    def num_local_params(self) -> int:
        def count(t: torch.Tensor) -> int:  # an mxfp4 code byte holds two parameters
            return 2 * t.numel() if ops.is_mxfp4(t) else t.numel()

        n = self.embed.numel() + (0 if self.cfg.tie_embeddings else count(self.lm_head))
        for L in self.layers:
            for k, v in L.items():
                if k.endswith(DERIVED):
                    continue
                if isinstance(v, tuple):
                    n += sum(t.numel() for t in v)
                else:
                    n += count(v)
        return n

    # ------------------------------------------------------------------ forward
    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        if self.tp == 1:
            if ids.is_cuda:
                return ops.embedding(ids, self.embed)
            return self.embed[ids.long()]
        x = ops.embedding(ids, self.embed, vocab_start=self.v_lo)
        return tp_all_reduce(x, self.ps)

    def _lora_slot(self, meta: AttnMeta) -> Optional[torch.Tensor]:
        """The step's adapter slots, where it has adapter rows and this model holds adapters."""
        return meta.lora_slot if self.lora is not None else None

    def _attention(self, L: dict, x: torch.Tensor, meta: AttnMeta, kv, li: int = -1) -> torch.Tensor:
        o = self._attn_core(L, x, meta, kv, li=li)
        y = ops.prefill_linear(o, L["wo"], wscale=self._wsc(L, "wo")) if "bo" not in L else F.linear(o, L["wo"])
        slot = self._lora_slot(meta)
        if slot is not None:
            ops.lora_add(self.lora, li, "wo", o, y, slot)
        if "bo" in L and self.rank == 0:
            y += L["bo"]
        return tp_all_reduce(y, self.ps)

    def _attn_core(self, L: dict, x: Optional[torch.Tensor], meta: AttnMeta, kv, slabs: Optional[tuple] = None,
                   rows: Optional[int] = None, rownorm: Optional[tuple] = None,
                   rowscale: Optional[tuple] = None, li: int = -1) -> torch.Tensor:
        """QKV projection, RoPE + KV-cache write, attention; returns the per-head output [T, Hq*D].
        ``slabs = (workspace, splits)``: decode QKV by the split-K skinny GEMM over ``x`` (row-major
        or fragment-packed with ``rows`` valid rows), reduced inside rope_and_cache; the attention
        output is then written fragment-packed for the o_proj skinny GEMM.  A step with adapter rows
        (``meta.lora_slot``; ``li`` = the layer's index) adds the adapters' qkv delta before the
        rotation: one more slab, or ops.lora_add on the plain projection's output."""
        c = self.cfg
        lslot = self._lora_slot(meta)
        k_cache, v_cache, kv_scale = (tuple(kv) + (None,))[:3] if kv is not None else (None, None, None)
        partial, ns = None, 0
        roped = False  # q / k already rotated by the qkv GEMM's epilogue
        T = rows if rows is not None else x.shape[0]
        cs = self.cos_sin if self.cos_sin is not None else _dummy_cs(self)
        if slabs is not None:
            ws, splits = slabs
            ns = self._proj_slabs(L, "wqkv", x, T, splits, rownorm)
            if lslot is not None:
                ns = ops.lora_slab(self.lora, li, "wqkv", x, T, ws, ns, lslot, rownorm=rownorm)
            if self._attn_rope and not meta.is_prefill and k_cache is not None and c.arch == "llama":
                # the attention kernel reduces the slabs, applies RoPE and writes the new k / v
                out = ops.packed_empty(T, self.hq * self.D, self.dtype, self.device)
                return ops.paged_decode_fused(ws, ns, meta.positions, cs, meta.slot_mapping, k_cache, v_cache,
                                              meta.block_tables, meta.seq_lens, self.hq, self.hkv, self.D, self.scale,
                                              workspace=meta.decode_ws, out=out, kv_scale=kv_scale)
            partial = ws
            qkv = torch.empty(T, ops.w_out(L["wqkv"]), dtype=self.dtype, device=self.device)
        elif "bqkv" in L:
            qkv = F.linear(x, L["wqkv"], L["bqkv"])
        elif c.arch == "llama" and self.D == 128 and self.cos_sin is not None and not c.qk_norm and lslot is None:
            # prefill-sized qkv on the tile kernel: RoPE of q / k fused into its epilogue (not for a
            # QK-norm model: its heads are normalised between the projection and the rotation, nor on
            # a step with adapter rows: the rotation comes after the adapters' delta)
            qkv, roped = ops.prefill_linear(x, L["wqkv"], rope=(meta.positions, cs, self.hq + self.hkv),
                                            rowscale=rowscale, wscale=self._wsc(L, "wqkv"))
        else:
            qkv = ops.prefill_linear(x, L["wqkv"], wscale=self._wsc(L, "wqkv"))
            if lslot is not None:
                ops.lora_add(self.lora, li, "wqkv", x, qkv, lslot)
        ops.rope_and_cache(qkv, meta.positions, cs, k_cache, v_cache,
                           meta.slot_mapping if k_cache is not None else None, self.hq, self.hkv, self.D,
                           apply_rope=c.arch == "llama" and not roped, partial=partial, nslabs=ns, kv_scale=kv_scale,
                           qk_norm=(L["q_norm"], L["k_norm"], c.norm_eps) if c.qk_norm else None)
        if meta.is_prefill:
            qb = (meta.qb_seq, meta.qb_start) if meta.qb_seq is not None else None
            paged = None
            if meta.ctx_start is not None:  # some prompts start with cached prefix blocks
                paged = (meta.ctx_start, k_cache, v_cache, meta.block_tables)
            nd = meta.num_decode
            if nd == 0:
                return ops.flash_prefill(qkv, meta.cu_seqlens, self.hq, self.hkv, self.D, self.scale, qblocks=qb,
                                         paged=paged, kv_scale=kv_scale)
            # mixed step: decode rows through paged_decode, prefill rows through flash prefill
            o = torch.empty(qkv.shape[0], self.hq * self.D, dtype=qkv.dtype, device=qkv.device)
            ops.paged_decode(qkv[:nd], k_cache, v_cache, meta.dec_block_tables, meta.dec_seq_lens, self.hq,
                             self.hkv, self.D, self.scale, workspace=meta.decode_ws, out=o[:nd], kv_scale=kv_scale)
            op = ops.flash_prefill(qkv[nd:], meta.cu_seqlens, self.hq, self.hkv, self.D, self.scale, qblocks=qb,
                                   paged=paged, out=o[nd:], kv_scale=kv_scale)
            if op.data_ptr() != o[nd:].data_ptr():  # CPU reference paths return a fresh tensor
                o[nd:] = op
        else:
            out = ops.packed_empty(T, self.hq * self.D, self.dtype, self.device) if slabs is not None else None
            o = ops.paged_decode(qkv, k_cache, v_cache, meta.block_tables, meta.seq_lens, self.hq, self.hkv,
                                 self.D, self.scale, workspace=meta.decode_ws, out=out, kv_scale=kv_scale)
        return o

    def _mlp(self, L: dict, x: torch.Tensor, meta: AttnMeta, li: int = -1) -> torch.Tensor:
        c = self.cfg
        if c.arch == "gpt2":
            h = ops.gelu_tanh(F.linear(x, L["w1"], L["b1"]))
            y = F.linear(h, L["w2"])
            if self.rank == 0:
                y += L["b2"]
            return tp_all_reduce(y, self.ps)
        if c.is_moe:
            if meta.is_prefill and self.tp > 1 and self.moe_comm == "a2a":
                return self._moe_a2a(L, x)
            if not meta.is_prefill and self.tp > 1 and self.moe_decode == "a2a":
                return self._moe_a2a_decode(L, x)
            return tp_all_reduce(self._moe(L, x, meta), self.ps)
        slot = self._lora_slot(meta)
        if slot is not None and "w13" in self.lora.dims:
            # adapter rows on gate / up: the delta enters before the activation, so the gate_up GEMM
            # runs plain, the delta is added in the resident row order and silu_mul pairs it up
            gu = (ops.prefill_linear(x, L["w13"], swiglu=False, wscale=self._wsc(L, "w13")) if self._w13_il
                  else F.linear(x, L["w13"]))
            ops.lora_add(self.lora, li, "w13", x, gu, slot)
            h = ops.silu_mul(gu, pairing={PACKED: 8, INTERLEAVED: 1}.get(self._layout, 0))
        elif self._w13_il:
            h = ops.prefill_linear(x, L["w13"], swiglu=self._swg, wscale=self._wsc(L, "w13"))
        else:
            h = ops.silu_mul(F.linear(x, L["w13"]), interleaved=False)
        y = ops.prefill_linear(h, L["w2"], wscale=self._wsc(L, "w2"))
        if slot is not None and "w2" in self.lora.dims:
            ops.lora_add(self.lora, li, "w2", h, y, slot)
        return tp_all_reduce(y, self.ps)

    def _moe(self, L: dict, x: torch.Tensor, meta: AttnMeta) -> torch.Tensor:
        """Top-k MoE over this rank's experts [e_lo, e_hi).  Tokens are sorted by expert (moe_align)
        and every local expert runs on its contiguous rows in ONE grouped launch per projection
        (gemm_tile.hip / moe_gemm.hip, device-side offsets: no host sync, so a decode step beyond
        the skinny kernels' row limit stays graph-capturable).  The CPU decode form is the
        dense-masked reference (every local expert on every token, scaled by its routing weight)."""
        c = self.cfg
        T = x.shape[0]
        K = c.top_k_experts
        ids, w, _ = ops.moe_router(x, L["router"], K, True)
        if not meta.is_prefill and not (self._moe_grouped and x.is_cuda):
            # CPU reference of the decode form (the GPU takes the routed grouped path below, which
            # needs no host sync either and runs only the (token, expert) pairs that were chosen)
            wd = torch.zeros(T, c.n_experts, dtype=torch.float32, device=x.device)
            wd.scatter_(1, ids.long(), w)
            out = torch.zeros(T, c.d_model, dtype=torch.float32, device=x.device)
            for j, e in enumerate(range(self.e_lo, self.e_hi)):
                h = ops.silu_mul(F.linear(x, self._expert(L, "w13", j)), interleaved=self._w13_il)
                out += F.linear(h, self._expert(L, "w2", j)).float() * wd[:, e:e + 1]
            return out.to(x.dtype)
        offsets, sorted_idx, inv_idx = ops.moe_align(ids, c.n_experts)
        xs = ops.gather_rows(x, sorted_idx, K)
        if self._moe_grouped and x.is_cuda:
            # every local expert in ONE grouped launch per projection, driven by the device-side
            # offsets (ops/csrc/moe_gemm.hip): no host sync, no per-expert loop
            offl = offsets[self.e_lo:self.e_hi + 1]
            part = self.tp > 1  # other ranks' experts' rows stay zero
            if self._w13_il:
                h = ops.moe_grouped_gemm(xs, L["w13"], offl, swiglu=self._swg, zero_fill=part)
            else:
                h = ops.silu_mul(ops.moe_grouped_gemm(xs, L["w13"], offl, zero_fill=part))
            ys = ops.moe_grouped_gemm(h, L["w2"], offl, zero_fill=part)
            return ops.moe_combine(ys, inv_idx, w, T)
        ys = torch.zeros_like(xs)
        off = offsets.tolist()  # one host sync per MoE layer (the per-expert hipBLASLt loop)
        for j, e in enumerate(range(self.e_lo, self.e_hi)):
            a, b = off[e], off[e + 1]
            if b > a:
                h = ops.silu_mul(F.linear(xs[a:b], self._expert(L, "w13", j)), interleaved=self._w13_il)
                ys[a:b] = F.linear(h, self._expert(L, "w2", j))
        return ops.moe_combine(ys, inv_idx, w, T)

    def _moe_a2a(self, L: dict, x: torch.Tensor) -> torch.Tensor:
        """Expert-parallel MoE with all-to-all dispatch / combine, for prefill
        at TP>1.  Activations arrive replicated (tensor-parallel attention); rank r routes its
        1/tp slice of the tokens, sends every (token, expert) row to the rank owning the expert,
        the owners sort what they received by local expert and run all local experts in one grouped
        GEMM launch per projection (host sync only for the all-to-all sizes), the results travel back by the reverse all-to-all, are combined with the
        routing weights, and the slices are all-gathered to the replicated layout the next layer's
        attention expects.  Decode keeps the graph-capturable replicated form (_moe + all-reduce):
        all-to-all splits are data-dependent and need a host sync."""
        c = self.cfg
        T, K, P, r = x.shape[0], c.top_k_experts, self.tp, self.rank
        epr = c.n_experts // P
        chunk = -(-T // P)
        t0, t1 = min(T, r * chunk), min(T, (r + 1) * chunk)
        n = t1 - t0
        xs = x[t0:t1]
        ids, w, _ = ops.moe_router(xs, L["router"], K, True)
        offsets, sorted_idx, inv_idx = ops.moe_align(ids, c.n_experts)
        send = ops.gather_rows(xs, sorted_idx, K) if n else xs.new_zeros(0, c.d_model)
        send_exp = ids.reshape(-1)[sorted_idx.long()].to(torch.int64)
        off = offsets.tolist()  # host sync: all-to-all split sizes
        send_counts = [off[(p + 1) * epr] - off[p * epr] for p in range(P)]
        cnt = torch.tensor(send_counts, dtype=torch.int64, device=x.device)
        rcnt = torch.empty_like(cnt)
        tp_all_to_all(rcnt, cnt, [1] * P, [1] * P, self.ps)
        recv_counts = rcnt.tolist()
        nrecv = sum(recv_counts)
        recv = x.new_empty(nrecv, c.d_model)
        tp_all_to_all(recv, send, recv_counts, send_counts, self.ps)
        recv_exp = torch.empty(nrecv, dtype=torch.int64, device=x.device)
        tp_all_to_all(recv_exp, send_exp, recv_counts, send_counts, self.ps)
        # the received rows arrive grouped by source rank; order them by local expert and run all
        # local experts in one grouped launch per projection (device offsets, no further sync)
        order = torch.argsort(recv_exp, stable=True)
        counts = torch.bincount(recv_exp[order] - self.e_lo, minlength=epr)
        loc_off = torch.zeros(epr + 1, dtype=torch.int32, device=x.device)
        loc_off[1:] = torch.cumsum(counts, 0).to(torch.int32)
        xs_l = recv[order]
        if self._w13_il:
            h = ops.moe_grouped_gemm(xs_l, L["w13"], loc_off, swiglu=self._swg, zero_fill=False)
        else:
            h = ops.silu_mul(ops.moe_grouped_gemm(xs_l, L["w13"], loc_off, zero_fill=False))
        y = torch.empty_like(recv)
        y[order] = ops.moe_grouped_gemm(h, L["w2"], loc_off, zero_fill=False)
        back = x.new_empty(n * K, c.d_model)
        tp_all_to_all(back, y, send_counts, recv_counts, self.ps)
        out = ops.moe_combine(back, inv_idx, w, n) if n else back[:0]
        if n < chunk:  # equal-size blocks for the all-gather
            out = torch.cat([out, out.new_zeros(chunk - n, c.d_model)])
        return tp_all_gather_rows(out, self.ps)[:T]

    def _a2a_equal(self, x: torch.Tensor) -> torch.Tensor:
        """All-to-all of equal blocks x [P, ...] -> out[p] = rank p's x[this rank]: the IPC kernel
        (custom_ar.hip, one launch, graph-capturable) on the GPU, else the group backend."""
        car = self.ps.custom_ar
        if car is not None and x.is_cuda and car.fits_a2a(x):
            return car.all_to_all(x)
        out = torch.empty_like(x)
        n = x.shape[0]
        tp_all_to_all(out.view(n, -1), x.reshape(n, -1), [1] * n, [1] * n, self.ps)
        return out

    def _moe_a2a_decode(self, L: dict, x: torch.Tensor) -> torch.Tensor:
        """Expert-parallel MoE for DECODE steps with static shapes, so the
        step stays capturable in a hipGraph: rank r routes its ceil(M/P) slice of the (replicated)
        rows; every (token, slot) pair goes to the rank owning its expert through a fixed-capacity
        all-to-all (cap = slice x top-k rows per rank pair, zero rows where a pair goes elsewhere;
        the IPC all-to-all kernel on the GPU, custom_ar.hip); the owner runs its local experts on
        what it received on the grouped skinny MFMA kernels (one launch for gate/up + SwiGLU of
        every local expert, one for their down projections into split-K slabs weighted one-hot by
        each row's expert - the slab sum IS the per-row expert selection), in chunks of up to 128
        rows (the row-major grouped kernel's 8-m-tile form: one weight stream per step at batch 64);
        the results return by the reverse all-to-all, are weighted and summed per token, and the
        slices are all-gathered.  Against the replicated form (every rank runs its experts on
        every token, then one all-reduce) it computes only routed pairs, streams the local expert
        weights once per 128-row chunk of the P x cap x K received rows (once per step at batch 64,
        TP 2), and moves two all-to-alls plus an all-gather; the replicated form stays the default
        (K8SLLM_MOE_DECODE=a2a selects this one)."""
        c = self.cfg
        P, r, K, d = self.tp, self.rank, c.top_k_experts, c.d_model
        epr = c.n_experts // P
        M = x.shape[0]
        cap = -(-M // P)
        if M < P * cap:
            x = torch.cat([x, x.new_zeros(P * cap - M, d)])
        xs = x[r * cap:(r + 1) * cap]
        ids, w, _ = ops.moe_router(xs, L["router"], K, True)  # [cap, K]
        ids = ids.long()
        npair = cap * K
        pair_x = xs.repeat_interleave(K, dim=0)  # [cap*K, d], pair j = (token j // K, slot j % K)
        dest = (ids // epr).view(-1)  # [cap*K]
        sel = dest.unsqueeze(0) == torch.arange(P, device=x.device).unsqueeze(1)  # [P, cap*K]
        send = pair_x.unsqueeze(0) * sel.unsqueeze(-1).to(x.dtype)
        # expert ids travel as bf16 (exact small integers, -1 = no pair), padded to 8 per block
        ne = -(-npair // 8) * 8
        send_e = torch.full((P, ne), -1.0, dtype=x.dtype, device=x.device)
        send_e[:, :npair] = torch.where(sel, (ids.view(-1) % epr).unsqueeze(0), torch.full_like(sel, -1,
                                                                                              dtype=torch.long)).to(x.dtype)
        recv = self._a2a_equal(send.contiguous())
        recv_e = self._a2a_equal(send_e)
        R = P * npair
        rows = recv.view(R, d)
        re = recv_e[:, :npair].reshape(-1).float()
        onehot = (re.unsqueeze(1) == torch.arange(epr, device=x.device, dtype=torch.float32).unsqueeze(0)).float()
        ws = self._skinny_ws
        if ws is not None and "w13_pg" not in L and "w13_dg" in L:
            # ONE_LAYOUT: the shared-A grouped decode GEMM over the packed experts, 64 rows a launch
            y = torch.empty(R, d, dtype=x.dtype, device=x.device)
            E = L["w13_dg"].shape[0]
            for c0 in range(0, R, ops.SKINNY_MAX_M):
                mc = min(ops.SKINNY_MAX_M, R - c0)
                act = torch.empty((E, -(-mc // 16), L["w13_dg"].shape[1] // 4, 64, 8), dtype=x.dtype, device=x.device)
                self._dec_grouped(L, "w13", ops.pack_activation(rows[c0:c0 + mc]), 2, mc, out=act)
                ns = self._dec_grouped(L, "w2", act, 0, mc, workspace=ws, row_w=onehot[c0:c0 + mc].contiguous())
                ops.reduce_slabs(ws, ns, mc, d, dtype=x.dtype, out=y[c0:c0 + mc])
        elif ws is not None and "w13_pg" in L:
            y = torch.empty(R, d, dtype=x.dtype, device=x.device)
            # up to 128 rows per grouped launch over the row-major expert weights: at decode batch
            # 64 and TP=2 the P x cap x top-k = 128 received rows stream each local expert ONCE
            step = (ops.SKINNY_GROUPED_MAX_M if L["w13_pg"].dim() == 3 and epr > 1 and x.is_cuda
                    else ops.SKINNY_MAX_M)
            for c0 in range(0, R, step):
                mc = min(step, R - c0)
                act = ops.skinny_grouped_swiglu(ops.pack_activation(rows[c0:c0 + mc]), L["w13_pg"], rows=mc)
                ns = ops.skinny_grouped_slabs(act, L["w2_pg"], ws, mc, onehot[c0:c0 + mc].contiguous(), splits=1)
                ops.reduce_slabs(ws, ns, mc, d, dtype=x.dtype, out=y[c0:c0 + mc])
        else:
            yf = torch.zeros(R, d, dtype=torch.float32, device=x.device)
            for j in range(epr):
                h = ops.silu_mul(F.linear(rows, self._expert(L, "w13", j)), interleaved=self._w13_il)
                yf += F.linear(h, self._expert(L, "w2", j)).float() * onehot[:, j:j + 1]
            y = yf.to(x.dtype)
        back = self._a2a_equal(y.view(P, npair, d))
        res = back[dest, torch.arange(npair, device=x.device)]  # [cap*K, d]
        z = (res.view(cap, K, d).float() * w.unsqueeze(-1)).sum(1).to(x.dtype)
        return tp_all_gather_rows(z, self.ps)[:M]

    def _norm(self, x: torch.Tensor, w) -> torch.Tensor:
        if isinstance(w, tuple):
            return ops.layer_norm(x, w[0], w[1], self.cfg.norm_eps)
        return ops.rms_norm(x, w, self.cfg.norm_eps)

    def forward(self, ids: torch.Tensor, meta: AttnMeta, kv_caches: Optional[list] = None) -> torch.Tensor:
        """Returns logits [rows, vocab_size] for the rows selected by ``meta.logits_idx`` (all rows
        when None)."""
        c = self.cfg
        if self._layout == LOADING:
            raise RuntimeError(f"{c.name}: a checkpoint load began (begin_load) and did not finish; load again")
        if meta.dec_src is not None:
            if (self.tp == 1 and ids.is_cuda and c.arch != "gpt2" and self._use_skinny(meta, ids)
                    and c.d_model % 512 == 0):
                # decode front end in one launch: ids -> embedding -> layer 0's deferred-norm operands
                residual, xw, ss = ops.embed_norm_partial(ids, self.embed, self.layers[0]["attn_norm"],
                                                          meta.dec_src, meta.dec_prev)
                return self._decode_layers_skinny(None, residual, meta, kv_caches, first=(xw, (ss, c.norm_eps)))
            ids = ops.resolve_ids(ids, meta.dec_src, meta.dec_prev)
        h = self.embed_tokens(ids)
        if c.arch == "gpt2":
            h = h + self.pos_embed[meta.positions.long()]
            residual = h
            for i, L in enumerate(self.layers):
                kv = kv_caches[i] if kv_caches is not None else None
                residual = residual + self._attention(L, self._norm(residual, L["ln1"]), meta, kv)
                residual = residual + self._mlp(L, self._norm(residual, L["ln2"]), meta)
            x = residual
            if meta.logits_idx is not None:
                x = x[meta.logits_idx]
            x = self._norm(x, self.final_norm)
        else:
            residual = h
            if self._use_skinny(meta, h):
                return self._decode_layers_skinny(None, residual, meta, kv_caches)
            # a step with adapter rows: the plain layer loop below, ops.lora_add after qkv, o and down
            lora = self._lora_slot(meta) is not None
            if not lora and self._fused_norm_ok(h):
                return self._head(self._prefill_fused_norm(residual, meta, kv_caches), meta)
            if not lora and meta.micro is not None and self.overlap_ok():
                return self._head(self._prefill_overlap(residual, meta, kv_caches), meta)
            x = ops.rms_norm(h, self.layers[0]["attn_norm"], c.norm_eps)
            n = len(self.layers)
            for i, L in enumerate(self.layers):
                kv = kv_caches[i] if kv_caches is not None else None
                if i + 1 == n and not lora and self._last_rows_ok(L, h, meta):
                    return self._head(self._last_rows(L, self._attn_core(L, x, meta, kv), residual, meta), meta)
                y = self._attention(L, x, meta, kv, li=i)
                x = ops.fused_add_rms_norm(y, residual, L["mlp_norm"], c.norm_eps)
                y = self._mlp(L, x, meta, li=i)
                if i + 1 < n:
                    x = ops.fused_add_rms_norm(y, residual, self.layers[i + 1]["attn_norm"], c.norm_eps)
                else:
                    if meta.logits_idx is not None:
                        y = y[meta.logits_idx]
                        residual = residual[meta.logits_idx].contiguous()
                    x = ops.fused_add_rms_norm(y.contiguous(), residual, self.final_norm, c.norm_eps)
        return self._head(x, meta)

    def overlap_ok(self) -> bool:
        """TP > 1 dense Llama prefill may run as two overlapped micro-batches (_prefill_overlap;
        K8SLLM_TP_OVERLAP=0 disables)."""
        return (self.tp > 1 and self.cfg.arch == "llama" and not self.cfg.is_moe and bool(self.layers)
                and "bqkv" not in self.layers[0] and os.environ.get("K8SLLM_TP_OVERLAP", "1") != "0")

    def _mlp_local(self, L: dict, x: torch.Tensor) -> torch.Tensor:
        """Dense SwiGLU MLP of this rank's F shard, before the row-parallel all-reduce."""
        if self._w13_il:
            h = ops.prefill_linear(x, L["w13"], swiglu=self._swg)
        else:
            h = ops.silu_mul(F.linear(x, L["w13"]), interleaved=False)
        return ops.prefill_linear(h, L["w2"])

    def _prefill_overlap(self, residual: torch.Tensor, meta: AttnMeta, kv_caches: Optional[list]) -> torch.Tensor:
        """Tensor-parallel prefill with the row-parallel all-reduces hidden behind compute
        (SURVEY.md §2.12 C-1 / C-2): the step's sequences form two micro-batches A and B (the
        runner's split, meta.micro) and every all-reduce is issued asynchronously (RCCL runs it on
        its own stream; the consumer waits on it just before use), so per layer

            attn A, o A, [AR A] | attn B, o B, [AR B] | norm A, mlp A, [AR2 A] | norm B, mlp B, [AR2 B]

        each all-reduce runs beside the other micro-batch's next compute segment (AR2 B beside the
        next layer's attention of A).  Row-wise the arithmetic is the serial form's: the same
        GEMMs, norms and sums per row, split by sequence (attention never crosses sequences)."""
        c = self.cfg
        eps = c.norm_eps
        mA, mB, TA = meta.micro
        metas = (mA, mB)
        rs = (residual[:TA], residual[TA:])
        x0 = ops.rms_norm(residual, self.layers[0]["attn_norm"], eps)
        xs = [x0[:TA], x0[TA:]]
        pend = [None, None]  # (y, work): a micro-batch's MLP output and its all-reduce in flight
        for i, L in enumerate(self.layers):
            kv = kv_caches[i] if kv_caches is not None else None
            ys, works = [None, None], [None, None]
            for b in (0, 1):
                if pend[b] is not None:
                    y2, w2 = pend[b]
                    w2.wait()
                    xs[b] = ops.fused_add_rms_norm(y2, rs[b], L["attn_norm"], eps)
                o = self._attn_core(L, xs[b], metas[b], kv)
                ys[b] = ops.prefill_linear(o, L["wo"])
                works[b] = tp_all_reduce_async(ys[b], self.ps)
            for b in (0, 1):
                works[b].wait()
                xb = ops.fused_add_rms_norm(ys[b], rs[b], L["mlp_norm"], eps)
                y2 = self._mlp_local(L, xb)
                pend[b] = (y2, tp_all_reduce_async(y2, self.ps))
        outs = []
        for b in (0, 1):
            y2, w2 = pend[b]
            w2.wait()
            idx = metas[b].logits_idx
            outs.append(ops.fused_add_rms_norm(y2[idx].contiguous(), rs[b][idx].contiguous(), self.final_norm, eps))
        return torch.cat(outs)

    def _fused_norm_ok(self, h: torch.Tensor) -> bool:
        """Dense Llama-family prefill at TP=1 on the tile GEMMs: the RMSNorms between projections
        can live in the GEMM epilogues (``_prefill_fused_norm``)."""
        c = self.cfg
        if not h.is_cuda or c.arch != "llama" or c.is_moe or self.tp != 1 or not self._w13_il:
            return False
        if c.qk_norm:  # the qkv GEMM's row scale exists only with its RoPE epilogue, which QK-norm rules out
            return False
        if self.D != 128 or self.cos_sin is None or any(k in self.layers[0] for k in ("bqkv", "bo")):
            return False
        L = self.layers[0]
        return ops.fused_norm_ok(h.shape[0], c.d_model, ops.w_out(L["wqkv"]), ops.w_in(L["wo"]), ops.w_out(L["w13"]),
                                 ops.w_in(L["w2"]))

    def _prefill_fused_norm(self, residual: torch.Tensor, meta: AttnMeta, kv_caches: Optional[list]) -> torch.Tensor:
        """The prefill layers with every RMSNorm but the first and the final one folded into the
        tile GEMMs: the o / down epilogues add their product to the residual stream in place and
        emit (residual * next norm weight, per-128-column sums of squares); qkv (+ RoPE) and
        gate_up (+ SwiGLU) scale their rows by the resulting 1/rms - no separate fused-add RMSNorm
        pass over the [tokens, d_model] activations between projections."""
        c = self.cfg
        eps = c.norm_eps
        n = len(self.layers)
        x = ops.rms_norm(residual, self.layers[0]["attn_norm"], eps)
        ss = None
        for i, L in enumerate(self.layers):
            kv = kv_caches[i] if kv_caches is not None else None
            o = self._attn_core(L, x, meta, kv, rowscale=(ss, eps) if ss is not None else None)
            if i + 1 == n and self.LAST_LAYER_ROWS and meta.logits_idx is not None:
                return self._last_rows_fused(L, o, residual, meta.logits_idx)
            x, ss = ops.gemm_tile_resid(o, L["wo"], residual, L["mlp_norm"], wscale=self._wsc(L, "wo"))
            act = ops.prefill_linear(x, L["w13"], swiglu=self._swg, rowscale=(ss, eps), wscale=self._wsc(L, "w13"))
            if i + 1 < n:
                x, ss = ops.gemm_tile_resid(act, L["w2"], residual, self.layers[i + 1]["attn_norm"],
                                            wscale=self._wsc(L, "w2"))
            else:
                y = ops.prefill_linear(act, L["w2"], wscale=self._wsc(L, "w2"))
                if meta.logits_idx is not None:
                    y = y[meta.logits_idx]
                    residual = residual[meta.logits_idx].contiguous()
                x = ops.fused_add_rms_norm(y.contiguous(), residual, self.final_norm, eps)
        return x

    def _last_rows_fused(self, L: dict, o: torch.Tensor, residual: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """The last layer of ``_prefill_fused_norm`` from the attention output ``o`` on, over the
        logit rows ``idx`` alone (LAST_LAYER_ROWS): the full-row form's tile GEMMs - o + residual,
        gate_up + SwiGLU with the row scale, down - launched on the gathered rows (the tile kernel
        and its epilogues treat every row alone: the same bits), then the final norm.  The GEMMs are
        called as tile GEMMs whatever the row count: fused_norm_ok routed the whole step there.
        No rows (a chunk that ends inside every prompt): nothing to compute."""
        eps = self.cfg.norm_eps
        if idx.numel() == 0:
            return residual.new_empty(0, residual.shape[1])
        o, res = o[idx].contiguous(), residual[idx].contiguous()
        x, ss = ops.gemm_tile_resid(o, L["wo"], res, L["mlp_norm"], wscale=self._wsc(L, "wo"))
        act = ops.gemm_tile(x, L["w13"], swiglu=self._swg, algo=ops.TILE_ALGO, rowscale=(ss, eps),
                            wscale=self._wsc(L, "w13"))
        y = ops.gemm_tile(act, L["w2"], algo=ops.TILE_ALGO, wscale=self._wsc(L, "w2"))
        return ops.fused_add_rms_norm(y, res, self.final_norm, eps)

    def _last_rows_ok(self, L: dict, h: torch.Tensor, meta: AttnMeta) -> bool:
        """``forward``'s layer loop may run its last layer's tail on the logit rows alone
        (``_last_rows``): a dense Llama at TP = 1 without biases whose o / gate_up / down take a GEMM
        with row-independent rows at any row count - the CPU forms, or on the GPU the tile kernel
        over fragment-packed (or encoded) weights, which prefill_linear sends there whatever the row
        count.  Row-major weights on the GPU go to hipBLASLt below TILE_MIN_M rows, whose choice of
        kernel (and so its rounding) depends on the row count: those keep the full-row form."""
        c = self.cfg
        if not self.LAST_LAYER_ROWS or meta.logits_idx is None or not meta.is_prefill:
            return False
        if c.arch != "llama" or c.is_moe or self.tp != 1 or "bo" in L:
            return False
        return not h.is_cuda or (self._w13_il and all(L[k].dim() == 4 for k in ("wo", "w13", "w2")))

    def _last_rows(self, L: dict, o: torch.Tensor, residual: torch.Tensor, meta: AttnMeta) -> torch.Tensor:
        """The last layer of ``forward``'s loop from the attention output ``o`` on, over the logit
        rows alone (``_last_rows_ok``), and the final norm: ``_attention``'s and ``_mlp``'s own calls
        on the gathered rows."""
        eps, idx = self.cfg.norm_eps, meta.logits_idx
        if idx.numel() == 0:
            return residual.new_empty(0, residual.shape[1])
        o, res = o[idx].contiguous(), residual[idx].contiguous()
        y = ops.prefill_linear(o, L["wo"], wscale=self._wsc(L, "wo"))
        x = ops.fused_add_rms_norm(y, res, L["mlp_norm"], eps)
        y = self._mlp(L, x, meta)
        return ops.fused_add_rms_norm(y.contiguous(), res, self.final_norm, eps)

    def _head(self, x: torch.Tensor, meta: AttnMeta) -> torch.Tensor:
        """Every exit of ``forward`` outside the decode fast path: ``x`` the final-normed rows
        (``meta.logits_idx``'s).  Embedding rows (``meta.pool_dim``) are pooled into ``meta.pooled``
        first; a step whose rows need no token (``want_logits`` False) skips the LM head."""
        if meta.pool_dim is not None:
            meta.pooled = ops.pool_l2(x, meta.pool_dim, out=meta.pooled)  # the caller's buffer, or a fresh one
        if not meta.want_logits:
            return x.new_empty(0, self.cfg.vocab_size)
        return self._logits(x)

    def _logits(self, x: torch.Tensor, rows: Optional[int] = None) -> torch.Tensor:
        """LM head (+ the TP all-gather of the vocab shards).  ``x``: the final-normed rows,
        row-major, or fragment-packed with ``rows`` valid rows (decode).  With a decode copy of the
        head (``lm_head_d``) up to dec_rows_max() rows at a time (128 for dense TP=1 models, else
        64) go through gemm_decode.hip, one stream of the head per launch - the decode step's and a
        prefill step's last-token logits alike; hipBLASLt otherwise."""
        if x.dim() == 2 and x.shape[0] == 0:  # a step without logit rows (a chunk that ends inside every prompt)
            return x.new_empty(0, self.cfg.vocab_size)
        hd, hq = self.lm_head_d, self.lm_head_q
        f8_only = hd is None and hq is not None  # the codes are the head's only decode form (_release_bf16)
        nv = (hd if hd is not None else hq).shape[0] * 16 if hd is not None or hq is not None else 0
        if x.dim() == 4:  # packed (decode): the decode copy (or the codes) exists by construction
            logits = torch.empty(rows, nv, dtype=self.dtype, device=self.device)
            self._dec(x, hd, hq, self.lm_head_qs, 1, rows, out=logits)
        elif nv and x.is_cuda and x.shape[0] <= self.dec_rows_max():
            logits = torch.empty(x.shape[0], nv, dtype=self.dtype, device=self.device)
            self._dec(ops.pack_activation(x), hd, hq, self.lm_head_qs, 1, x.shape[0], out=logits)
        elif self.lm_head.dim() == 4 or f8_only:
            # ONE_LAYOUT: the packed head (or its codes) is the only copy - dec_rows_max()-row chunks
            M, mc = x.shape[0], self.dec_rows_max()
            logits = torch.empty(M, nv, dtype=self.dtype, device=self.device)
            for i in range(0, M, mc):
                m = min(mc, M - i)
                if f8_only:
                    self._dec(ops.pack_activation(x[i:i + m]), None, hq, self.lm_head_qs, 1, m, out=logits[i:i + m])
                else:
                    ops.dec_gemm(ops.pack_activation(x[i:i + m]), hd, 1, m, out=logits[i:i + m])
        else:
            logits = F.linear(x, self.lm_head)
        logits = tp_all_gather_last(logits, self.ps)
        if self.vocab_padded != self.cfg.vocab_size:
            logits = logits[:, : self.cfg.vocab_size]
        return logits

    # ------------------------------------------------------------------ fused decode tail
    # Row ceiling of the decode fast path for the models whose every projection runs on the dense
    # shared-A decode GEMM (dec_rows_max).  Tests and tools set it to 64 for the routing before the
    # 128-row kernels (A/B runs); values above ops.DEC_MAX_M are clamped.
    DEC_ROWS_MAX = 128

    def dec_rows_max(self) -> int:
        """Most rows a decode step may have and stay on the skinny path (_decode_layers_skinny):
        min(DEC_ROWS_MAX, ops.DEC_MAX_M) = 128 for a dense model at TP=1 whose layers hold wqkv_d /
        wo_d / w13_d / w2_d and whose head has its decode copy (every GEMM of the step is then
        ops.dec_gemm, with a 65..128-row configuration for each shape); 64 otherwise - MoE (the
        grouped launches), TP > 1 (the IPC fused tail and its staging), gemm_skinny weights."""
        if not self._dec_wide:
            return ops.SKINNY_MAX_M
        return max(ops.SKINNY_MAX_M, min(int(self.DEC_ROWS_MAX), ops.DEC_MAX_M))

    def _dec_wide_ok(self) -> bool:
        c = self.cfg
        if self.tp != 1 or c.is_moe or not self.layers:
            return False
        L = self.layers[0]
        # (decode copy or None, codes or None, epilogue): a projection may hold its codes only
        ws = [(L.get(k + "_d"), L.get(k + "_q"), 2 if k == "w13" else 0) for k in PROJ]
        ws.append((self.lm_head_d, self.lm_head_q, 1))
        if any(wd is None and wq is None for wd, wq, _ in ws):
            return False
        return all(ops.dec_config(*ops.skinny_wdims(wd if wd is not None else wq), epi, rows=ops.DEC_MAX_M,
                                  f8=wd is None) is not None for wd, wq, epi in ws)

    def _use_skinny(self, meta: AttnMeta, h: torch.Tensor) -> bool:
        """Llama-family decode steps of up to dec_rows_max() rows (128 for dense TP=1 models on the
        shared-A decode GEMM, 64 otherwise) run every projection through the decode GEMMs over
        fragment-packed weights (see _init_skinny)."""
        if self._skinny_ws is None or not self._lora_w13_skinny_ok(meta):
            return False
        return (not meta.is_prefill and h.shape[0] <= self.dec_rows_max()
                and meta.logits_idx is None and self.SKINNY_DECODE)

    def _lora_w13_skinny_ok(self, meta: AttnMeta) -> bool:
        """A step with adapter rows over a gate_up arena stays on the skinny decode loop where the
        gate_up launch can take the delta before its SwiGLU epilogue: gemm_decode over the PACKED
        w13 (the arena's B rows are in its order), at most 16 deferred-norm sums per row.  Otherwise
        - gemm_skinny's w13_p, the INTERLEAVED two-copy layout - the step takes the generic layer
        loop, as row counts above the limit do."""
        if self._lora_slot(meta) is None or "w13" not in self.lora.dims:
            return True
        L = self.layers[0]
        return (self._layout == PACKED and self._lora_w13_layout == PACKED and ("w13_d" in L or "w13_q" in L)
                and self.cfg.d_model // 512 <= 16)

    def _init_skinny(self) -> None:
        """(Re)build everything derived from the weights: the resident layout of the projections
        (module docstring) and the decode path's views, copies and workspace.  Whatever layout
        the model is in, each layer first drops its derived tensors and then moves its projections,
        through their canonical form, to the row-major layout this model serves from - INTERLEAVED
        for Llama-family models whose F is a multiple of 64, else CANONICAL - so peak residency is
        the model plus one layer's projections; after ``begin_load`` the loader's tensors are
        CANONICAL.  The row-major tensors then serve decode through gemm_skinny_rm_kernel
        (ops/csrc/gemm_skinny.hip: whole 128-B lines by LDS-DMA; a shape it does not take gets
        fragment-packed ``*_p`` copies), and ``_init_dec`` adds the decode GEMM's packed copies or,
        under ``ONE_LAYOUT``, makes them the only copy (PACKED).

        Per layer at decode (5-7 launches): qkv skinny (split-K slabs) -> paged_decode_fused (slab
        reduce, RoPE, KV write, attention) -> o skinny (slabs) -> add_norm_partial (residual add,
        deferred mlp norm) -> gate_up skinny with the SwiGLU epilogue -> down skinny (slabs) ->
        add_norm_partial.  TP>1: each row-parallel o / down tail is ONE launch with the IPC
        all-reduce (slab sum + all-reduce + residual add + RMSNorm + packed A: _tp_tail); over
        RCCL, reduce_slabs + all-reduce + fused_add_rms_norm + pack_activation.
        On the CPU the same ops run as fp32 references with the kernels' split-K slicing, so the
        control flow (and TP over gloo) is covered by the CPU tests."""
        c = self.cfg
        if self.lm_head.dim() == 4:  # before the head's scales go: an fp8-only head dequantises with them
            self.lm_head = self.canonical_head().contiguous()
        self._skinny_ws = self.lm_head_d = self.lm_head_q = self.lm_head_qs = None
        self._rc_o, self._dec_wide, self._attn_rope = 0, False, False
        ff = c.ffn_dim if c.is_moe else self.f_local  # experts are sharded by count (EP), not by F
        old = CANONICAL if self._layout == LOADING else self._layout
        new = INTERLEAVED if c.arch == "llama" and ff % 64 == 0 else CANONICAL
        d, nq = c.d_model, (self.hq + 2 * self.hkv) * self.D
        dec = (c.arch == "llama" and self.SKINNY_DECODE and new == INTERLEAVED
               and not (d % 64 or nq % 64 or (self.hq * self.D) % 32))
        for L in self.layers:
            if not dec:  # no _init_dec below: fp8-only projections back to bf16 here (else there, layer by layer)
                self._remat(L, new)
            self._drop_derived(L)
            if old != new:
                for key in PROJ:
                    if not ops.is_codes(L[key]):
                        L[key] = relayout(L[key], key, old, new).contiguous()
        self._layout = new
        if not dec:
            self._lora_relayout()
            return
        # (In-launch split-K epilogues - RoPE + KV write in the qkv GEMM, residual add + norm
        # producer in the o / down GEMMs, reduced by each tile's last-arriving workgroup - measured
        # 5-6 us per layer-op SLOWER than the slab GEMM + separate reduce kernel on the row-major
        # kernel too (profiles/r03/fused_epilogues_rowmajor.jsonl) and were removed.)
        # decode RoPE + KV write inside the attention kernel (paged_decode_fused), reading the qkv
        # GEMM's split-K slabs directly: one launch per layer fewer - where ops.PD_FORMS has a fused
        # row for this head dim and group (the same rows for a bf16 and an fp8 cache); else
        # rope_and_cache + the unfused kernel
        # (a QK-norm model normalises its heads in rope_and_cache: no fused row does that)
        self._attn_rope = not c.qk_norm and ops.paged_decode_why(self.D, self.hq // self.hkv, fused=True) is None
        rowmajor = (self.hq * self.D) % 64 == 0
        self.skinny_layout = "rowmajor" if rowmajor else "packed"
        for L in self.layers:
            for key in PROJ:  # MoE: stacked per local expert for the grouped (grid.z = expert) launches
                if ops.is_codes(L[key]):  # codes-only so far: _init_dec's _remat makes its view
                    continue
                sfx = "_pg" if L[key].dim() == 3 else "_p"
                L[key + sfx] = L[key] if rowmajor else _each(L[key], ops.pack_skinny)
        split = ops.SKINNY_SPLITS_FORCE  # 0: the launcher picks per call (kernel and batch dependent)
        self._split_qkv = self._split_o = self._split_d = split
        self._init_dec()
        self._dec_wide = self._dec_wide_ok()
        self._lora_relayout()
        self._skinny_ws = torch.empty(self._skinny_ws_numel(), dtype=torch.float32, device=self.device)
        self.set_decode_fusion()

    def _skinny_ws_numel(self) -> int:
        """fp32 elements of the split-K slab workspace every decode projection shares: the most
        slabs x output columns of any projection, times the most rows a step can have.  The most
        slabs of an [N, K] projection is taken over every row count up to the limit: gemm_skinny's
        automatic split (row dependent up to 64 rows) and, where the layers hold decode copies,
        gemm_dec's configuration in every row class (ops.dec_row_classes) up to the CEILING of
        dec_rows_max() - DEC_MAX_M for a model on the wide path - not what DEC_ROWS_MAX says at
        the moment, so flipping that switch at run time stays inside the buffer.  MoE: the expert
        down projections write one slab group per local expert, and the EP all-to-all decode runs
        up to SKINNY_GROUPED_MAX_M received rows per grouped launch.  With resident LoRA adapters
        (enable_lora) every dense projection has room for one more slab: an adapter's delta; the
        gate_up delta (enable_lora(mlp=True)) is one [rows, 2F] image at the start of the workspace."""
        c, split = self.cfg, self._split_qkv
        d, nq, no = c.d_model, (self.hq + 2 * self.hkv) * self.D, self.hq * self.D
        dec_rows = ops.DEC_MAX_M if self._dec_wide else ops.SKINNY_MAX_M
        # decode copies, or - where a projection is fp8-only - its codes
        dec_copies = bool(self.layers) and any(k.endswith(DEC_COPIES + ("_q",)) for k in self.layers[0])
        f8 = bool(self.layers) and any(k.endswith("_q") for k in self.layers[0])

        def most(N: int, K: int) -> int:
            s = split if split else max(ops.skinny_auto_splits(m, N, K) for m in (1, 33, 64))
            for r in (r for r in ops.dec_row_classes() if dec_copies and r <= dec_rows):
                for enc in (({}, self._enc_kw()) if f8 else ({},)):  # the fp8 / mxfp4 encoding may pick another split
                    cfg = ops.dec_config(N, K, 0, rows=r, **enc)
                    s = max(s, cfg[0] if cfg else 1)
            return s

        extra = 1 if self.lora is not None else 0  # an adapter's delta is one more slab (ops.lora_slab)
        if c.is_moe:
            mlp = (self.e_hi - self.e_lo) * ops.skinny_nslabs(c.ffn_dim, 1) * d
        else:
            mlp = (most(d, self.f_local) + extra) * d
        n = max((most(nq, d) + extra) * nq, (most(d, no) + extra) * d, mlp)
        if self.lora is not None and "w13" in self.lora.dims:
            n = max(n, 2 * self.f_local)
        return n * (ops.SKINNY_GROUPED_MAX_M if c.is_moe else dec_rows)

    # decode buckets up to this many rows take the row-complete o projection by default: per decode
    # step 1.4 % faster at 1-2 rows, 0.9 % at 4-16, 0.4 % at 32 (profiles/r05/rc_rows_ab.jsonl;
    # batch-1 TPOT 3.14 vs 3.18 ms, latency_b1_rc_ab.md); at 64 rows its per-workgroup re-read of
    # the attention output cancels the gain (neutral)
    RC_O_MAX_ROWS = 32

    def set_decode_fusion(self, rc=None) -> None:
        """The row-complete o projection as the alternative to the decode step's first
        add_norm_partial launch (profiles/r05/README.md; bit-compatible with the slab path): the o
        projection without split-K slabs, residual add and the gate_up GEMM's norm operands in its
        epilogue (ops.dec_gemm_rc).  At 64 rows it is neutral (re-reading the attention output
        from L2 in every workgroup costs what the slab round trip did); at 1-32 rows it wins
        0.4-1.4 % per step, so ``rc=None`` (the default) turns it on for decode buckets of at most
        RC_O_MAX_ROWS rows (the hipGraphs are captured per bucket, so the choice is static per
        graph); True: every bucket; False: off.  Needs TP=1 and the decode weight copies.
        (Measured and removed in round 6's cleanup: the add-RMSNorm as the consuming GEMM's first
        phase behind a grid seam - neutral to slower - and the down projection row-complete -
        0.2-4.5 % slower at 4-32 rows; profiles/r05/README.md.)"""
        c = self.cfg
        if rc is True and self.layers and any(ops.is_codes(self.layers[0][k]) for k in ("wo", "w13")):
            raise ValueError(f"the row-complete o projection reads bf16 weights: wo / w13 are resident as "
                             f"{self.DEC_WEIGHTS} only (prefill_weights={self.PREFILL_WEIGHTS})")
        ok = (self.tp == 1 and not c.is_moe and bool(self.layers) and "w13_d" in self.layers[0]
              and c.d_model % 512 == 0)
        # fp8 decode weights: the row-complete kernel reads bf16 and leaves the gate_up GEMM the wide
        # deferred norm, which has no fp8 form - o and gate_up (3/4 of a layer's bytes with it)
        # would stay on the bf16 encoding, so the default there is off
        dflt = 0 if ok and "w13_q" in self.layers[0] else self.RC_O_MAX_ROWS
        rows = dflt if rc is None else (1 << 30 if rc is True else int(rc))
        self._rc_o = rows if ok and "wo_d" in self.layers[0] else 0

    def _decode_layers_skinny(self, x: torch.Tensor, residual: torch.Tensor, meta: AttnMeta,
                              kv_caches: Optional[list], first: Optional[tuple] = None) -> torch.Tensor:
        """Activations between the skinny GEMMs travel fragment-packed (whole-line A loads): the
        attention output (paged_decode) and the MLP activation (SwiGLU epilogue) are written in the
        A-operand layout, and every RMSNorm is deferred: add_norm_partial writes residual * w plus
        per-row partial sums of squares, and the consuming GEMM scales its outputs by 1/rms."""
        c, ws, n = self.cfg, self._skinny_ws, len(self.layers)
        eps = c.norm_eps
        M = residual.shape[0]
        lslot = self._lora_slot(meta)  # adapter rows: every adapted projection gets one more slab
        # first = layer 0's (A operand, rownorm), already produced with the embedding (embed_norm_partial)
        xw, rn = first if first is not None else self._norm_tail(residual, None, 0, self.layers[0]["attn_norm"])
        for i, L in enumerate(self.layers):
            kv = kv_caches[i] if kv_caches is not None else None
            op = self._attn_core(L, xw, meta, kv, slabs=(ws, self._split_qkv), rows=M, rownorm=rn, li=i)
            rc = None
            if M <= self._rc_o and "w13_d" in L and lslot is None:  # (no slab for an adapter's delta to join)
                # o projection row-complete: residual += o and the gate_up GEMM's normed input in
                # the same launch (no split-K slabs, no add_norm launch)
                rc = ops.dec_gemm_rc(op, L["wo_d"], M, residual, L["mlp_norm"], eps)
            if rc is None:
                ns = self._proj_slabs(L, "wo", op, M, self._split_o)
                if lslot is not None:
                    ns = ops.lora_slab(self.lora, i, "wo", op, M, ws, ns, lslot)
                if c.is_moe and self.tp > 1 and self.moe_decode == "a2a":
                    # EP all-to-all MoE: residual += o (all-reduced), then the complete, replicated
                    # MLP output comes back from _moe_a2a_decode
                    xn = self._tp_tail(ws, ns, residual, L["mlp_norm"], packed=False)
                    if xn is None:
                        xn = ops.fused_add_rms_norm(self._row_parallel_sum(ws, ns, M, residual), residual,
                                                    L["mlp_norm"], eps)
                    z = self._moe_a2a_decode(L, xn)
                    nw = self.layers[i + 1]["attn_norm"] if i + 1 < n else self.final_norm
                    xr = ops.fused_add_rms_norm(z, residual, nw, eps)
                    if i + 1 < n:
                        xw, rn = ops.pack_activation(xr), None
                        continue
                    return self._logits(xr)
                if c.is_moe:
                    ns = self._moe_skinny(L, residual, ws, ns, M)
                    if i + 1 < n:
                        xw, rn = self._norm_tail(residual, ws, ns, self.layers[i + 1]["attn_norm"], rows=M)
                    continue
                rc = self._norm_tail(residual, ws, ns, L["mlp_norm"], rows=M)
            xw, rn = rc  # the dense MLP's input, from either form of the o projection
            if "w13_d" in L or "w13_q" in L:
                act = ops.packed_empty(M, self.f_local, self.dtype, self.device)
                dkw = {}
                if lslot is not None and "w13" in self.lora.dims:
                    # the adapters' gate_up delta, one fp32 [M, 2F] image in the packed w13's row order
                    # at the start of the workspace - free here: _norm_tail has consumed the o slabs
                    # and the down GEMM writes after the gate_up launch has read it (stream order)
                    ops.lora_slab(self.lora, i, "w13", xw, M, ws, 0, lslot, rownorm=rn)
                    dkw = dict(delta=ws, delta_slot=lslot, delta_slots=self.lora.slots)
                self._dec(xw, L.get("w13_d"), L.get("w13_q"), L.get("w13_qs"), 2, M, out=act, rownorm=rn, **dkw)
            else:
                act = ops.skinny_swiglu(xw, L["w13_p"], rows=M, packed_out=True, rownorm=rn)
            ns = self._proj_slabs(L, "w2", act, M, self._split_d)
            if lslot is not None:
                ns = ops.lora_slab(self.lora, i, "w2", act, M, ws, ns, lslot)
            if i + 1 < n:
                xw, rn = self._norm_tail(residual, ws, ns, self.layers[i + 1]["attn_norm"], rows=M)
        # final norm feeds the LM head: fragment-packed for the decode GEMM (gemm_decode.hip), or
        # complete and row-major for hipBLASLt where no decode copy of the head exists
        packed = self.lm_head_d is not None or self.lm_head_q is not None
        x = self._tp_tail(ws, ns, residual, self.final_norm, packed=packed)
        if x is None:
            y = self._row_parallel_sum(ws, ns, M, residual)
            if y is None:
                out = (ops.packed_empty(M, residual.shape[1], residual.dtype, residual.device) if packed
                       else torch.empty_like(residual))
                x = ops.reduce_add_rms_norm(out, residual, ws, ns, self.final_norm, eps)
            else:
                x = ops.fused_add_rms_norm(y, residual, self.final_norm, eps)
                if packed:
                    x = ops.pack_activation(x)
        return self._logits(x, rows=M)

    def _moe_skinny(self, L: dict, residual: torch.Tensor, ws, ns: int, M: int) -> int:
        """MoE decode MLP on the grouped skinny kernels: residual += the o
        projection; the router reads the complete RMSNorm; ONE launch runs gate/up + SwiGLU of every
        local expert over every row (grid.z = expert; at decode batch sizes every expert is selected
        by some row, so the step streams every expert's weights either way), ONE launch runs their
        down projections into slabs scaled by the routing weights (0 where an expert was not
        chosen) - the caller's residual-add kernel summing the slabs is the expert combine.  Host
        sync free, so the step stays in the decode hipGraph."""
        c = self.cfg
        xn = self._tp_tail(ws, ns, residual, L["mlp_norm"], packed=False)
        xp = None  # the normed rows fragment-packed (the expert GEMMs' A operand)
        if xn is None:
            y = self._row_parallel_sum(ws, ns, M, residual)
            if y is None:
                # TP=1: one launch writes the router's row-major rows and the packed A operand
                xp = ops.packed_empty(M, c.d_model, self.dtype, self.device)
                xn = ops.reduce_add_rms_norm(torch.empty_like(residual), residual, ws, ns, L["mlp_norm"], c.norm_eps,
                                             packed_out=xp)
            else:
                xn = ops.fused_add_rms_norm(y, residual, L["mlp_norm"], c.norm_eps)
        _, _, wd = ops.moe_router(xn, L["router"], c.top_k_experts, True)
        if xp is None:
            xp = ops.pack_activation(xn)
        if "w13_dg" in L and M <= ops.SKINNY_MAX_M:  # shared-A decode GEMM over the packed expert copies
            E = L["w13_dg"].shape[0]
            act = torch.empty((E, -(-M // 16), L["w13_dg"].shape[1] // 4, 64, 8), dtype=self.dtype, device=self.device)
            self._dec_grouped(L, "w13", xp, 2, M, out=act)
            return self._dec_grouped(L, "w2", act, 0, M, workspace=ws, row_w=wd[:, self.e_lo:self.e_hi].contiguous())
        act = ops.skinny_grouped_swiglu(xp, L["w13_pg"], rows=M)
        return ops.skinny_grouped_slabs(act, L["w2_pg"], ws, M, wd[:, self.e_lo:self.e_hi].contiguous(), splits=1)

    def _proj_slabs(self, L: dict, key: str, x: Optional[torch.Tensor], rows: int, split: int,
                    rownorm: Optional[tuple] = None) -> int:
        """Split-K slabs of a decode projection into the shared workspace: the shared-A decode
        GEMM over the packed copy ``L[key + "_d"]`` where one exists, else gemm_skinny over
        ``L[key + "_p"]``.  Returns the slab count."""
        wd, wq = L.get(key + "_d"), L.get(key + "_q")
        if wd is not None or wq is not None:  # wd None: the codes are the only copy
            return self._dec(x, wd, wq, L.get(key + "_qs"), 0, rows, workspace=self._skinny_ws, rownorm=rownorm)
        return ops.skinny_slabs(x, L[key + "_p"], self._skinny_ws, split, rows=rows, rownorm=rownorm)

    @staticmethod
    def _dec(x: torch.Tensor, wd: torch.Tensor, wq: Optional[torch.Tensor], wqs: Optional[torch.Tensor], epi: int,
             rows: int, rownorm: Optional[tuple] = None, **kw) -> int:
        """ops.dec_gemm over the fp8 or mxfp4 encoding (``wq``, ``wqs``) of a weight where one exists and
        gemm_decode.hip has an fp8 form for the shape at ``rows`` rows with this deferred norm (the
        wide form of the row-complete o projection's sums reads bf16), else over the bf16 copy
        ``wd`` - the same values either way, so the choice is one of speed only.  ``wd`` None: the
        weight is resident as its codes only (_f8_only_ok made sure every launch has an fp8 form;
        one without raises in ops.dec_gemm)."""
        if wq is not None and (wd is None or not (rownorm is not None and rownorm[0].shape[1] > 16)):
            N, K = ops.skinny_wdims(wq)
            if wd is None or ops.dec_config(N, K, epi, rows=rows, **ops.enc_kw(wq)) is not None:
                return ops.dec_gemm(x, wq, epi, rows, rownorm=rownorm, wscale=wqs, **kw)
        return ops.dec_gemm(x, wd, epi, rows, rownorm=rownorm, **kw)

    def prefill_encodings(self) -> dict:
        """What prefill reads each dense projection and the head from: "fp8" / "mxfp4" where the codes
        are the only resident copy (the bf16 copy is released), "bf16" otherwise; layer 0 speaks for all."""
        L = self.layers[0] if self.layers else {}
        enc = {k: ops.enc_name(L[k]) for k in PROJ if k in L}
        enc["head"] = ops.enc_name(self.lm_head_q) if self.lm_head_d is None else "bf16"
        return enc

    def decode_encodings(self) -> dict:
        """Which encoding each decode projection streams from ("fp8" | "mxfp4" | "bf16" per key of
        wqkv, wo, w13, w2, head) where the decode GEMM has both; layer 0 speaks for all."""
        L = self.layers[0] if self.layers else {}
        name = lambda wq: "bf16" if wq is None else "mxfp4" if ops.is_mxfp4(wq) else "fp8"  # noqa: E731
        enc = {k: name(L.get(k + "_q")) for k in PROJ if k in L}
        enc["head"] = name(self.lm_head_q)
        return enc

    def _enc_kw(self) -> dict:
        """dec_config's keyword for this model's quantised decode encoding."""
        return ops.enc_kw(self.DEC_WEIGHTS)

    def _want_dec(self) -> set:
        """Which projections gemm_decode.hip gets in its fragment-packed form (``DECODE_GEMM`` =
        auto | dec | rm): a subset of {"head", "attn", "mlp", "experts"}.  Every one where
        ONE_LAYOUT applies - the packed tensors become the only copy (PACKED), at no extra memory
        at any size - and on the CPU.  Otherwise (INTERLEAVED plus packed copies) auto weighs the
        copies against the device, W being the weights' bytes: the LM head always (<= 2.1 GB,
        Llama-3-70B); the attention projections while W + their copies fit 70 % of the device; a
        dense MLP while 2W fits half of it (Llama-3-8B: 16 GB of 288; Llama-3-70B at TP=1, 141 GB,
        would keep its MLP on the row-major skinny kernel); MoE experts while 2W fits 70 %
        (Mixtral-8x7B at TP=1: 93 + 93 GB)."""
        mode = self.DECODE_GEMM
        if mode in ("rm", "0", "off") or self.cfg.arch != "llama":
            return set()
        if mode in ("dec", "1", "on") or self.device.type != "cuda" or self._one_layout_wanted():
            return {"head", "attn", "mlp", "experts"}
        total = torch.cuda.get_device_properties(self.device).total_memory
        w = self.num_local_params() * 2
        attn = sum((L["wqkv"].numel() + L["wo"].numel()) * 2 for L in self.layers)
        parts = {"head"}
        if w + attn <= 0.7 * total:
            parts.add("attn")
        if self.cfg.is_moe:
            if 2 * w <= 0.7 * total:
                parts.add("experts")
        elif 2 * w <= total // 2:
            parts.add("mlp")
        return parts

    def _one_layout_wanted(self) -> bool:
        """ONE_LAYOUT applies: a Llama-family model (dense or MoE) whose projections all have a
        decode configuration (the shapes are the same in every layer, so layer 0 decides)."""
        c = self.cfg
        if not (self.ONE_LAYOUT and c.arch == "llama" and self.layers and self.SKINNY_DECODE
                and self.DECODE_GEMM not in ("rm", "0", "off")
                and (self.device.type == "cuda" or self.ONE_LAYOUT == "force")):
            return False
        L = self.layers[0]
        if L["wqkv"].dim() != 2 or L["w13"].dim() != (3 if c.is_moe else 2):
            return False
        (nq, d), (f2, _) = L["wqkv"].shape, L["w13"].shape[-2:]
        attn = ops.dec_available(nq, d, 0) and ops.dec_available(d, nq - 2 * self.hkv * self.D, 0)
        if c.is_moe:  # every local expert on the grouped (grid.z = expert) decode GEMM and the grouped tile GEMM
            E = L["w13"].shape[0]
            mlp = (ops.dec_config(f2, d, 2, experts=E) is not None
                   and ops.dec_config(d, f2 // 2, 0, experts=E) is not None)
        else:
            mlp = ops.dec_available(f2, d, 2) and ops.dec_available(d, f2 // 2, 0)
        return attn and mlp and d % 256 == 0 and f2 % 256 == 0

    def _expert(self, L: dict, key: str, j: int) -> torch.Tensor:
        """Local expert j's weight row-major as the per-expert fallback paths read it (w13 in the
        ``_w13_il`` pairing), whatever the resident layout (ONE_LAYOUT: packed [E, N/16, K/32, 64, 8])."""
        return relayout(L[key][j], key, self._layout, INTERLEAVED if self._packed else self._layout)

    def canonical_head(self) -> torch.Tensor:
        """The LM head as row-major [vocab shard, d] (ONE_LAYOUT keeps only its packed copy)."""
        h = self.lm_head
        if ops.is_codes(h):  # the codes are the only copy: the bf16 values they were quantised from
            return ops.dequantize_codes(h, self.lm_head_qs, self.dtype)
        return ops.unpack_skinny(h) if h.dim() == 4 else h

    def canonical(self, L: dict, key: str) -> torch.Tensor:
        """A dense projection as the row-major [out, in] weight of the reference / the checkpoint
        format (w13 as [gate; up]), whatever its resident layout (row-major, gate/up interleaved
        per 128 rows, or the one fragment-packed copy)."""
        if key not in PROJ:  # norm weights (attn_norm, mlp_norm, q_norm, k_norm): stored as they are
            return L[key]
        return to_canonical(L[key], key, self._layout, L.get(key + "_qs"), self.dtype)

    @torch.no_grad()
    def copy_weights_from(self, src: "CausalLM") -> None:
        """Copy ``src``'s weights into this model (same config and TP shard; any device / dtype /
        resident layout on either side - the projections go through their canonical form), then
        rebuild what this model derives from them.  Used to give an fp32 CPU reference the GPU
        model's exact weights."""
        self.embed.copy_(src.embed)
        if self.lm_head is not self.embed:
            h = src.canonical_head().to(self.lm_head.device)
            if ops.is_codes(self.lm_head):  # codes-only head: straight to codes and scales
                _, q, qs = ops.encode_weight(h.to(self.dtype), self.DEC_WEIGHTS)
                self.lm_head.copy_(q)
                self.lm_head_qs.copy_(qs)
            else:
                self.lm_head.copy_(ops.pack_skinny(h) if self.lm_head.dim() == 4 else h)
        for a, b in zip(self.final_norm if isinstance(self.final_norm, tuple) else (self.final_norm,),
                        src.final_norm if isinstance(src.final_norm, tuple) else (src.final_norm,)):
            a.copy_(b)
        derived = False
        for Ld, Ls in zip(self.layers, src.layers):
            for k, v in Ld.items():
                if k.endswith(DERIVED):
                    derived = True
                elif k in PROJ and ops.is_codes(v):
                    # codes-only here: the source's canonical values straight to codes and scales, one
                    # projection's bf16 at a time
                    q, qs = self._codes(src.canonical(Ls, k).to(device=v.device, dtype=self.dtype), k)
                    v.copy_(q)
                    Ld[k + "_qs"].copy_(qs)
                elif k in PROJ and ops.is_codes(Ls[k]):
                    v.copy_(to_resident(src.canonical(Ls, k), k, self._layout))
                elif k in PROJ:
                    v.copy_(relayout(Ls[k], k, src._layout, self._layout))
                elif isinstance(v, tuple):
                    for a, b in zip(v, Ls[k]):
                        a.copy_(b)
                else:
                    v.copy_(Ls[k])
        # what is derived from the copied weights is stale now: under PACKED the layers' derived keys
        # ARE the weights and only a tied head keeps a separate packed copy (of the embedding)
        # (an fp8-decoding model requantises: its bf16 weights become the new dequantised values)
        if self.DEC_WEIGHTS in ("fp8", "mxfp4"):
            self._f8_defer = False  # the weights are real now, whatever the model was built with
            self._init_skinny()
        elif self._packed and self.lm_head_d is not None and self.lm_head_d is not self.lm_head:
            self.lm_head_d.copy_(ops.pack_skinny(self.lm_head))
        elif derived and not self._packed:
            self._init_skinny()

    def _init_dec(self) -> None:
        """Packed copies for the shared-A decode GEMM, per projection where gemm_decode has a
        launch configuration for its shape (ops.dec_config): wqkv_d / wo_d / w2_d
        ([N/16, K/32, 64, 8]), w13_d (gate/up interleaved per 16 rows as [8 gate | 8 up]), and the
        LM head; MoE expert stacks w13_dg / w2_dg ([E, ...], grid.z = expert).  Where ONE_LAYOUT
        applies (``_one_layout_wanted``) each layer adopts its packed copies as the weights before
        the next layer is packed (peak memory = the weights + one layer's copy) and the model ends
        PACKED; otherwise it stays INTERLEAVED and prefill keeps reading the row-major tensors.

        ``DEC_WEIGHTS`` = "fp8": every dense projection (and the head) that gets a packed copy and
        has an fp8 decode configuration is first quantised per output row, its resident tensor
        overwritten with the dequantised values (so the packed copy, prefill and the checkpoint
        hold exactly what the fp8 kernel computes with; a tied embedding table with them), and its
        codes and scales kept as ``*_q`` / ``*_qs`` in the packed copy's row order - layer by
        layer, so peak memory stays the model plus one layer.  MoE expert stacks that get packed
        copies are quantised too, expert by expert (``_quantize_experts``: 5-d stacks of codes and
        scales under ``w13_q`` / ``w13_qs`` / ``w2_q`` / ``w2_qs``), where the grouped launch has a
        form over the encoding for both projections (ops.dec_grouped_q_config); else they stay bf16.
        ``DEC_WEIGHTS`` = "mxfp4": the same with ops.quantize_mxfp4 (one scale per row and block of
        32 along K, so the [8 gate | 8 up] row interleave carries codes and block scales along
        unchanged), the packed codes and block scales (ops.pack_skinny_f4) under the same two keys.

        ``PREFILL_WEIGHTS`` = "fp8" / "mxfp4" on top (of the same DEC_WEIGHTS): each ONE_LAYOUT layer then releases the packed bf16
        tensor of every projection ``_f8_only_ok`` accepts - the codes become ``L[key]`` itself
        (``_release_bf16``) - before the next layer is touched, and so does the head.  A model that
        already holds fp8-only projections (a second ``_init_skinny``, a weight copy) turns each
        layer's back to bf16 first (``_remat``), one layer at a time."""
        if self.layers:
            self._remat(self.layers[0], self._layout)  # layer 0's shapes decide below
        parts, one = self._want_dec(), self._one_layout_wanted()
        f8 = self.DEC_WEIGHTS in ("fp8", "mxfp4") and not self._f8_defer
        bf16_experts = None  # why the expert stacks stay on bf16, where they do
        f8_only = f8 and self.PREFILL_WEIGHTS == self.DEC_WEIGHTS  # codes-only, in either encoding
        why = None  # why nothing can be codes-only, if so
        if f8_only and (self.cfg.is_moe or self.tp != 1 or not one):
            why = "MoE" if self.cfg.is_moe else "TP > 1" if self.tp != 1 else "not ONE_LAYOUT-packed"
        ceil = self._dec_row_ceiling(parts) if f8_only and why is None else 0
        stayed: dict = {}
        for L in self.layers:
            self._remat(L, self._layout)
            for key in ("wqkv", "wo", "w2", "w13"):  # w13 (three passes of temporaries) last: a fixed allocation order
                w = L[key]
                if w.dim() == 3:  # an [E, ...] stack for the grouped launches: both projections or neither
                    E, F2, d = L["w13"].shape
                    sfx, ok = "_dg", "experts" in parts and all(
                        ops.dec_config(n, k, epi, experts=E) is not None for n, k, epi in ((F2, d, 2), (d, F2 // 2, 0)))
                    if f8:  # the codes beside the packed stack: both projections or neither, as for _dg
                        bf16_experts = "no packed expert copies" if not ok else self._experts_q_why(E, F2, d)
                        if bf16_experts is None:
                            self._quantize_experts(L, key)
                else:
                    sfx, ok = "_d", (("attn" if key in ("wqkv", "wo") else "mlp") in parts
                                     and ops.dec_available(*w.shape, 2 if key == "w13" else 0))
                if ok and f8 and sfx == "_d":
                    self._quantize_fp8(L, key)
                if ok:
                    L[key + sfx] = relayout(w, key, self._layout, PACKED)
            if one:
                self._adopt_packed(L)
            if f8_only:
                for key in PROJ:
                    r = why or self._f8_only_why(L.get(key + "_q"), 2 if key == "w13" else 0, ceil)
                    if r is None:
                        self._release_bf16(L, key)
                    else:
                        stayed[key] = r
        N, K = self.lm_head.shape
        if "head" in parts and N % 16 == 0 and K % 32 == 0 and ops.dec_available(N, K, 1):
            if f8 and self._f8_shape_ok(N, K, 1):
                deq, self.lm_head_q, self.lm_head_qs = ops.encode_weight(self.lm_head, self.DEC_WEIGHTS)
                self.lm_head.copy_(deq)  # tied: the embedding too
                del deq
            r = (why or self._f8_only_why(self.lm_head_q, 1, ceil)) if f8_only else "off"
            if r is None:
                # the codes are the head's only copy: an untied bf16 head goes; a tied one stays as
                # what it also is, the embedding table, and only its packed decode copy is not made
                if self.lm_head is not self.embed:
                    self.lm_head = self.lm_head_q
            else:
                if f8_only:
                    stayed["head"] = r
                self.lm_head_d = ops.pack_skinny(self.lm_head)
                if one and self.lm_head is not self.embed:
                    self.lm_head = self.lm_head_d  # ONE_LAYOUT: the packed head is the only copy too
        elif f8_only:
            stayed["head"] = why or "no decode copy of the head"
        if one:
            self._layout = PACKED
        if bf16_experts:
            log.info("%s: decode_weights=%s leaves the MoE expert stacks on bf16 (%s)", self.cfg.name,
                     self.DEC_WEIGHTS, bf16_experts)
        if stayed:
            log.info("%s: prefill_weights=%s keeps the bf16 copy of %s", self.cfg.name, self.PREFILL_WEIGHTS,
                     ", ".join(f"{k} ({r})" for k, r in stayed.items()))

    def _dec_row_ceiling(self, parts: set) -> int:
        """The most rows a decode step of this model will have once built (dec_rows_max's ceiling):
        DEC_MAX_M where every projection and the head have a decode configuration at that many
        rows (what _dec_wide_ok will find), else SKINNY_MAX_M.  From the shapes, before any layer
        is packed."""
        L = self.layers[0]
        shapes = [tuple(L[k].shape) + (2 if k == "w13" else 0,) for k in PROJ if L[k].dim() == 2]
        N, K = self.lm_head.shape
        wide = (len(shapes) == 4 and "head" in parts and N % 16 == 0 and K % 32 == 0
                and all(ops.dec_available(n, k, e, rows=ops.DEC_MAX_M) for n, k, e in shapes + [(N, K, 1)]))
        return ops.DEC_MAX_M if wide else ops.SKINNY_MAX_M

    @staticmethod
    def _f8_only_why(wq: Optional[torch.Tensor], epi: int, ceil: int) -> Optional[str]:
        """None when the weight with the codes ``wq`` (fp8 or mxfp4) may be resident as those only,
        else why not: it needs the encoding, a decode form over it in every row class up to the
        model's row ceiling (nothing may ever ask for the bf16 copy) and the tile GEMM's form over it."""
        if wq is None:
            return "no quantised encoding"
        N, K = ops.skinny_wdims(wq)
        enc, kw = ops.enc_name(wq), ops.enc_kw(wq)
        if not all(ops.dec_config(N, K, epi, rows=r, **kw) is not None for r in ops.dec_row_classes() if r <= ceil):
            return f"no {enc} decode form in some row class"
        return None if ops.tile_codes_ok(wq) else f"no {enc} form of the prefill GEMM for the shape"

    @staticmethod
    def _release_bf16(L: dict, key: str) -> None:
        """PACKED layer: the codes of ``key`` become the resident weight; its packed bf16 tensor
        (``L[key]`` and ``*_d``, one tensor) is released."""
        L[key] = L[key + "_q"]
        del L[key + "_d"]

    def _codes(self, w: torch.Tensor, key: str) -> tuple:
        """(packed codes, scales in packed row order) of the CANONICAL weight ``w`` of ``key``."""
        return ops.encode_weight(w, self.DEC_WEIGHTS, key == "w13")[1:]

    def _remat(self, L: dict, form: str) -> None:
        """Every codes-only projection of the layer back to a bf16 tensor in the row-major layout
        ``form`` (the dequantised values - what it was quantised from), its codes dropped, with the
        gemm_skinny view ``*_p`` the other projections got in _init_skinny."""
        for key in PROJ:
            if ops.is_codes(L.get(key)):
                w = to_resident(self.canonical(L, key), key, form).contiguous()
                L[key] = w
                del L[key + "_q"], L[key + "_qs"]
                L[key + "_p"] = w if self.skinny_layout == "rowmajor" else ops.pack_skinny(w)

    def _f8_shape_ok(self, N: int, K: int, epi: int) -> bool:
        """gemm_decode.hip has a form over this model's quantised encoding (fp8 or mxfp4) for the
        weight [N, K] in some row class."""
        return any(ops.dec_config(N, K, epi, rows=r, **self._enc_kw()) is not None for r in ops.dec_row_classes())

    def _quantize_fp8(self, L: dict, key: str) -> None:
        """The fp8 encoding of the dense projection ``L[key]`` (resident row-major, INTERLEAVED or
        CANONICAL): the tensor is overwritten in place with the dequantised values (the gemm_skinny
        view ``*_p`` aliases it; a packed ``*_p`` copy is refreshed) and ``*_q`` / ``*_qs`` hold
        the codes, fragment-packed, and the scales in the row order of the packed copy ``*_d``
        (w13: [8 gate | 8 up] per 16 rows - a row permutation, which per-row scales follow)."""
        w = L[key]
        N, K = w.shape
        if not self._f8_shape_ok(N, K, 2 if key == "w13" else 0):
            return
        # (block scales run along K and row scales with their rows, so the row order is free: the
        # canonical rows are quantised, codes and scales permuted into the packed copy's row order)
        deq, L[key + "_q"], L[key + "_qs"] = ops.encode_weight(to_canonical(w, key, self._layout), self.DEC_WEIGHTS,
                                                               key == "w13")
        w.copy_(to_resident(deq, key, self._layout))
        p = L.get(key + "_p")
        if p is not None and p is not w:
            L[key + "_p"] = ops.pack_skinny(w)

    def _experts_q_why(self, E: int, F2: int, d: int) -> Optional[str]:
        """None when the grouped decode GEMM has a form over this model's quantised encoding for
        both expert projections ([E, F2, d] gate_up and [E, d, F2 / 2] down), else why not."""
        for name, (n, k, epi) in (("gate_up", (F2, d, 2)), ("down", (d, F2 // 2, 0))):
            if ops.dec_grouped_q_config(n, k, epi, E, **self._enc_kw()) is None:
                return f"no {self.DEC_WEIGHTS} grouped form, or none faster than bf16, for {name} [{E}, {n}, {k}]"
        return None

    def _quantize_experts(self, L: dict, key: str) -> None:
        """The fp8 / mxfp4 encoding of the expert stack ``L[key]`` ([E, out, in], row-major,
        INTERLEAVED or CANONICAL), one expert at a time (the fp32 temporaries stay one expert's):
        each expert's rows are overwritten in place with the dequantised values (a row-major
        ``*_pg`` view aliases them; a packed ``*_pg`` copy is refreshed) and ``*_q`` / ``*_qs``
        hold the stacks of packed codes [E, out/16, in/64 | in/128, 64, 16] and of scales ([E, out]
        fp32 | [E, out/16, in/128, 16, 4] uint8) in the row order of the packed copy ``*_dg``
        (w13: [8 gate | 8 up] per 16 rows, the scales permuted with the rows).  The codes kept are
        those of the dequantised values: where a row's (block's) largest element rounded down to
        half the code range, the first pass's scale is one step coarser than the one the values
        themselves ask for - the same values on either, but only the second is what a checkpoint
        load, a weight copy or a second ``_init_skinny`` will find, so those reproduce the codes."""
        w = L[key]
        Q = S = None  # the [E, ...] stacks, allocated from expert 0's shapes
        pg = L.get(key + "_pg")
        for e in range(w.shape[0]):
            c = to_canonical(w[e], key, self._layout)
            deq, q, s = ops.encode_weight(c, self.DEC_WEIGHTS, key == "w13", settle=True)  # see the docstring
            w[e].copy_(to_resident(deq, key, self._layout))
            if pg is not None and pg is not w:
                pg[e].copy_(ops.pack_skinny(w[e]))
            if Q is None:
                Q, S = (torch.empty((w.shape[0],) + t.shape, dtype=t.dtype, device=t.device) for t in (q, s))
            Q[e].copy_(q)
            S[e].copy_(s)
            del c, deq, q, s
        L[key + "_q"], L[key + "_qs"] = Q, S

    @staticmethod
    def _dec_grouped(L: dict, key: str, a: torch.Tensor, epi: int, rows: int, **kw) -> int:
        """The grouped (grid.z = expert) decode GEMM of the expert stack ``key``: over its fp8 or
        mxfp4 codes (``*_q`` / ``*_qs``) where the layer holds them and ops.dec_grouped_q_config
        has a form for the stack, else over the packed bf16 stack ``*_dg`` - the same values
        either way, so the choice is one of speed only (the grouped analogue of ``_dec``)."""
        wq = L.get(key + "_q")
        if wq is not None:
            E, N, K = ops.grouped_q_wdims(wq)
            if ops.dec_grouped_q_config(N, K, epi, E, **ops.enc_kw(wq)) is not None:
                return ops.dec_gemm_grouped_q(a, wq, L[key + "_qs"], epi, rows, **kw)
        return ops.dec_gemm_grouped(a, L[key + "_dg"], epi, rows, **kw)

    @staticmethod
    def _adopt_packed(L: dict) -> None:
        """ONE_LAYOUT: the layer's packed decode copies become its weights; the row-major tensors
        go with the gemm_skinny views that still referenced them."""
        for key in PROJ:
            L[key] = L[key + ("_dg" if key + "_dg" in L else "_d")]
            L.pop(key + "_p", None)
            L.pop(key + "_pg", None)

    def _tp_tail(self, ws, ns: int, residual: torch.Tensor, norm_w, packed: bool) -> Optional[torch.Tensor]:
        """TP>1 on the GPU with the IPC all-reduce: the row-parallel tail (slab sum, all-reduce,
        residual add, RMSNorm, the next GEMM's input layout) as ONE fused launch
        (custom_ar.hip car_fused_tail_kernel); None where it does not apply."""
        car = self.ps.custom_ar
        M, d = residual.shape
        if self.tp == 1 or ns == 0 or car is None or not residual.is_cuda or not car.fits_tail(M, d):
            return None
        out = (ops.packed_empty(M, d, residual.dtype, residual.device) if packed
               else torch.empty_like(residual))
        return car.fused_tail(ws, ns, residual, norm_w, self.cfg.norm_eps, out, packed)

    def _row_parallel_sum(self, ws, ns: int, M: int, residual: torch.Tensor) -> Optional[torch.Tensor]:
        """TP>1: the row-parallel projection's slabs summed to bf16 and all-reduced; None at TP=1."""
        if self.tp == 1 or ns == 0:
            return None
        y = ops.reduce_slabs(ws, ns, M, residual.shape[1], dtype=residual.dtype)
        return tp_all_reduce(y, self.ps)

    def _norm_tail(self, residual: torch.Tensor, ws, ns: int, norm_w, rows: Optional[int] = None) -> tuple:
        """residual += the projection's slabs; returns (A operand for the next skinny GEMM, rownorm)."""
        eps = self.cfg.norm_eps
        xp = self._tp_tail(ws, ns, residual, norm_w, packed=True)
        if xp is not None:
            return xp, None
        y = self._row_parallel_sum(ws, ns, residual.shape[0], residual)
        if y is not None:  # TP>1: all-reduced partial sums, complete norm, packed A
            return ops.pack_activation(ops.fused_add_rms_norm(y, residual, norm_w, eps)), None
        if residual.shape[1] % 512 == 0:
            xw, ss = ops.add_norm_partial(residual, ws, ns, norm_w)
            return xw, (ss, eps)
        out = ops.packed_empty(residual.shape[0], residual.shape[1], residual.dtype, residual.device)
        return ops.reduce_add_rms_norm(out, residual, ws, ns, norm_w, eps), None


_DUMMY_CS: dict = {}


def _dummy_cs(m: CausalLM) -> torch.Tensor:
    k = (m.device, m.D)
    if k not in _DUMMY_CS:
        _DUMMY_CS[k] = torch.zeros(1, m.D, dtype=torch.float32, device=m.device)
    return _DUMMY_CS[k]
