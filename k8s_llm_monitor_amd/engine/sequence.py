"""Request / sequence state for the continuous-batching engine."""
from __future__ import annotations

import enum
import itertools
import time
from dataclasses import dataclass, field
from typing import Optional

import numpy as np


@dataclass
class SamplingParams:
    """Defaults follow the reference's ``llm`` block (``internal/config/config.go:141-145``):
    max_tokens 2000, temperature 0.1."""

    max_tokens: int = 2000
    temperature: float = 0.1
    top_k: int = 0
    top_p: float = 1.0
    ignore_eos: bool = False
    stop_token_ids: tuple = ()
    # sampling penalties (ops/reference.py apply_penalties), neutral by default: the repetition
    # penalty (> 0) scales the logits of tokens in the prompt or the answer so far; presence and
    # frequency are subtracted for tokens of the answer so far (once / per occurrence)
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    # token log-probabilities (ops/reference.py token_logprobs): of each answer token under the
    # model's distribution - before penalties, temperature and top-k / top-p - and of the
    # ``top_logprobs`` (0..20, needs ``logprobs``) most likely alternatives; Sequence.output_logprobs
    logprobs: bool = False
    top_logprobs: int = 0
    # constrained decoding (engine/guide.py): plain data, one of {"choice": [str, ...]},
    # {"regex": str}, {"json_schema": dict}; the answer then matches it in full when it finishes
    # with "stop" (cut by max_tokens or the deadline it may be an incomplete match)
    guide: Optional[dict] = None
    # per-request LoRA: the name of a configured adapter (EngineConfig.lora_adapters), None = the base model
    adapter: Optional[str] = None

    def has_penalties(self) -> bool:
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0


class SeqStatus(enum.Enum):
    WAITING = "waiting"
    RUNNING = "running"
    FINISHED = "finished"
    ABORTED = "aborted"


_ids = itertools.count()


@dataclass
class Sequence:
    prompt_ids: list[int]
    params: SamplingParams
    request_id: str = ""
    seq_id: int = field(default_factory=lambda: next(_ids))
    output_ids: list[int] = field(default_factory=list)
    # for a sequence that asked (SamplingParams.logprobs), aligned with output_ids: per token
    # (lp, [(id, lp), ...]) - its log-probability and the top_logprobs alternatives; else None
    output_logprobs: Optional[list] = None
    status: SeqStatus = SeqStatus.WAITING
    block_table: list[int] = field(default_factory=list)
    finish_reason: Optional[str] = None
    # timing (seconds, time.perf_counter clock)
    t_arrival: float = field(default_factory=time.perf_counter)
    t_first_token: Optional[float] = None
    t_finish: Optional[float] = None
    n_preemptions: int = 0
    num_cached: int = 0  # leading prompt tokens whose KV came from the prefix cache (this admission)
    # chunked prefill: tokens whose KV is in the cache (prefix cache + prefill chunks run so far),
    # the chunk the current prefill step computes, and whether the whole prompt has been prefilled
    num_computed: int = 0
    chunk: int = 0
    prefilled: bool = False
    # pipelined prefill: id of the in-flight prefill step whose sampled token will be this
    # sequence's first output token (its prompt is fully computed, the token not yet read back);
    # 0 = none.  Reset whenever the sequence's blocks are freed (preemption, abort, finish).
    pending_first: int = 0
    user: object = None  # opaque payload for the caller (future, callback, ...)
    deadline: Optional[float] = None  # time.perf_counter() by which the answer is due (engine.add_request)
    guide: object = None  # the compiled engine.guide.Guide of params.guide (engine.add_request)
    # per-request LoRA (engine.add_request): the adapter's slot in the model's arena (-1: the base
    # model) and the seed of its prefix-cache hash chain (0: the base model's hashes)
    lora_slot: int = -1
    hash_seed: int = 0
    # embedding requests (engine.add_request embed=): the width asked for (0: a generation request)
    # and the result - the first embed_dim entries of the last token's final-normed hidden row,
    # L2-normalised, fp32; None until the sequence finishes with finish_reason "embed"
    embed_dim: int = 0
    embedding: Optional[np.ndarray] = None

    @property
    def num_tokens(self) -> int:
        return len(self.prompt_ids) + len(self.output_ids)

    @property
    def all_ids(self) -> list[int]:
        return self.prompt_ids + self.output_ids

    @property
    def last_token(self) -> int:
        return self.output_ids[-1] if self.output_ids else self.prompt_ids[-1]

    def timings(self) -> dict:
        end = self.t_finish or time.perf_counter()
        ttft = (self.t_first_token - self.t_arrival) if self.t_first_token else None
        n = len(self.output_ids)
        decode_s = (end - self.t_first_token) if self.t_first_token else 0.0
        return {
            "prompt_tokens": len(self.prompt_ids),
            "completion_tokens": n,
            "latency_ms": round((end - self.t_arrival) * 1e3, 3),
            "ttft_ms": round(ttft * 1e3, 3) if ttft is not None else None,
            "decode_tokens_per_s": round((n - 1) / decode_s, 2) if n > 1 and decode_s > 0 else None,
            "preemptions": self.n_preemptions,
        }
