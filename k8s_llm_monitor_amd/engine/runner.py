"""Model runner: owns the paged KV cache, turns a StepPlan into device tensors, runs the model
and samples.

Decode steps are replayed from hipGraphs (``torch.cuda.CUDAGraph`` is hipGraph on ROCm) captured
once per batch-size bucket.  A bucket's graph reads static device buffers (token ids, positions,
slot mapping, block tables, sequence lengths, sampling parameters, RNG state) that the host
refreshes with a handful of async copies before each replay; the only host<->device sync per
step is reading back the sampled token ids.  Prefill runs eagerly (variable shapes).

KV-cache layouts are the ones the HIP kernels are written for (``ops/csrc/rope_cache.hip``):
K ``[NB, Hkv, D/8, 16, 8]`` and V ``[NB, Hkv, D, 16]`` per layer, one allocation for all layers
sized from ``kv_cache_gb`` (MI355X: 288 GB HBM per GPU - an 8B model leaves >250 GB for KV).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import ops
from ..models.llama import AttnMeta, CausalLM
from .sequence import Sequence

BLOCK_SIZE = 16
KV_CACHE_DTYPES = ("bf16", "fp8")
DEFAULT_BUCKETS = (1, 2, 4, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256)


@dataclass
class RunnerConfig:
    max_num_seqs: int = 64
    max_model_len: int = 8192
    kv_cache_gb: float = 16.0  # <= 0: max_num_seqs x max_model_len worth of blocks
    num_blocks: Optional[int] = None  # overrides kv_cache_gb
    use_graphs: bool = True
    seed: int = 0
    kv_cache_dtype: str = "bf16"  # "fp8": e4m3 codes + per-token scales (ops.kv_cache_alloc)


class ModelRunner:
    def __init__(self, model: CausalLM, cfg: RunnerConfig):
        self.model = model
        self.cfg = cfg
        self.device = model.device
        c = model.cfg
        self.max_len = min(cfg.max_model_len, c.max_position)
        self.max_blocks_per_seq = (self.max_len + BLOCK_SIZE - 1) // BLOCK_SIZE
        L, hkv, D = c.n_layers, model.hkv, model.D
        if cfg.kv_cache_dtype not in KV_CACHE_DTYPES:
            raise ValueError(f"kv_cache_dtype must be one of {KV_CACHE_DTYPES}, not {cfg.kv_cache_dtype!r}")
        self.kv_cache_dtype = cfg.kv_cache_dtype
        fp8 = cfg.kv_cache_dtype == "fp8"
        why = ops.paged_decode_why(D, None, f8=True) if fp8 and self.device.type == "cuda" else None
        if why is not None:  # no fp8 form for this head dim, whatever the group
            raise ValueError(f"kv_cache_dtype 'fp8': {why}")
        kv_dtype = torch.float8_e4m3fn if fp8 else model.dtype
        per_block = ops.kv_bytes_per_block(L, hkv, D, kv_dtype)  # K + V over all layers (+ scales for fp8)
        if cfg.num_blocks:
            nb = cfg.num_blocks
        elif cfg.kv_cache_gb <= 0:  # auto: every admitted sequence can reach max_len (+ one spare block)
            nb = cfg.max_num_seqs * self.max_blocks_per_seq + 1
        else:
            nb = max(self.max_blocks_per_seq + 1, int(cfg.kv_cache_gb * (1 << 30) // per_block))
        self.num_blocks = nb
        self.k_cache, self.v_cache, *sc = ops.kv_cache_alloc(L, nb, hkv, D, kv_dtype, self.device)
        self.kv_scale = sc[0] if sc else None
        self.kv_cache_bytes = nb * per_block
        self.kv = [(self.k_cache[i], self.v_cache[i], self.kv_scale[i] if fp8 else None) for i in range(L)]
        self.is_gpu = self.device.type == "cuda"
        B = cfg.max_num_seqs
        self.B = B
        dev = self.device
        # static decode inputs (graph inputs): views of ONE device buffer laid out like the pinned
        # host staging (_Staging), so a step's inputs go over in a single host-to-device copy
        self.d_all = torch.zeros(_Staging.size(B, self.max_blocks_per_seq), dtype=torch.int32, device=dev)
        (self.d_ids, self.d_src, self.d_pos, self.d_slots, self.d_lens, self.d_topk, self.d_temp, self.d_topp,
         self.d_bt) = _Staging.views(self.d_all, B, self.max_blocks_per_seq)
        self.d_src.fill_(-1)
        self.d_slots.fill_(-1)
        self.d_topp.fill_(1.0)
        self.rng = torch.tensor([cfg.seed, 0], dtype=torch.int64, device=dev)
        self.d_out = torch.zeros(B, dtype=torch.int32, device=dev)
        # sampling penalties: the device-resident state (ops.PenaltyState, allocated by the first
        # request that asks for a penalty), the sequences' slots in it, and the decode rows' slots -
        # a graph input of its own (not part of the staging buffer: it changes only when the batch
        # does), all -1 until the feature is used
        self.pen: Optional[ops.PenaltyState] = None
        self._pen_slot: dict[int, int] = {}  # seq_id -> slot
        self._pen_free: list[int] = []
        self.d_pslot = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self._pslot_sent = np.full(B, -1, dtype=np.int32)  # what d_pslot holds (as of the last upload)
        # constrained decoding: the device-resident guide state (ops.GuideState, allocated by the
        # first guided request), the sequences' slots in it and the decode rows' slots - a graph
        # input of its own like d_pslot, all -1 until the feature is used
        self.gd: Optional[ops.GuideState] = None
        self._gd_slot: dict[int, int] = {}  # seq_id -> slot
        self._gd_free: list[int] = []
        self.d_gslot = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self._gslot_sent = np.full(B, -1, dtype=np.int32)  # what d_gslot holds (as of the last upload)
        # token log-probabilities (ops.token_logprobs), off until the first request asks
        # (logprob_enable): the rows' packed records, what each decode row wants (-1: nothing; a
        # graph input of its own like d_pslot) and the pinned buffers a step's records are read
        # back into, beside the tokens
        self.lp_on = False
        self.d_lp: Optional[torch.Tensor] = None
        self.d_want: Optional[torch.Tensor] = None
        self._want_sent = np.full(B, -1, dtype=np.int32)  # what d_want holds (as of the last upload)
        self.h_lp: list = [None, None]
        self._pf_lp: list = [None, None]  # pinned records of in-flight prefill steps
        # per-request LoRA (lora_setup, once adapters are configured): the decode rows' adapter slots -
        # a graph input of its own like d_pslot - and a second set of decode graphs for steps with
        # adapter rows, captured from the first adapter request on (lora_enable); a step without an
        # adapter row replays the plain graphs
        self.d_lslot: Optional[torch.Tensor] = None
        self._lslot_sent = None
        self.lora_on = False
        self.graphs_lora: dict[int, list] = {}
        # embedding requests (ops.pool_l2 after the final norm of a prefill step), off until the
        # first one (embed_enable): prefill steps then stage the rows' embedding widths, the pooled
        # rows go into one device buffer (grown on demand; steps are ordered on the stream) and are
        # read back into one of two pinned fp32 buffers, beside the tokens
        self.embed_on = False
        self._d_emb: Optional[torch.Tensor] = None
        self._pf_emb: list = [None, None]
        self.decode_ws = ops.decode_workspace(B, model.hq, D, self.max_blocks_per_seq * BLOCK_SIZE, dev, model.hkv) \
            if self.is_gpu else None
        # pinned host staging, double-buffered: with pipelined decode the host fills step N+1's
        # inputs while step N's host-to-device copies may still be queued
        self.stage = [_Staging(B, self.max_blocks_per_seq, self.is_gpu, idx=i) for i in range(2)]
        # the staging copy as the first node of each decode graph (one graph per staging buffer and
        # bucket): a replay then starts with its own inputs instead of a separate copy in front of it
        # (removes a ~100 us launch gap per decode step between the copy and the graph's first
        # kernel; profiles/r03/README.md)
        self.graph_h2d = True
        self._stage_i = 0
        self.h_out = [torch.zeros(B, dtype=torch.int32, pin_memory=self.is_gpu) for _ in range(2)]
        self._out_i = 0
        self._pf_bufs = [None, None]  # pinned prefill-input staging (_pf_stage)
        self._pf_i = 0
        self._pf_out = [None, None]  # pinned sampled tokens of in-flight prefill steps
        self._pf_oi = 0
        self.buckets = [b for b in DEFAULT_BUCKETS if b < B] + [B]
        self.graphs: dict[int, list] = {}  # bucket -> [graph] (or one graph per staging buffer)
        self.graph_pool = None
        self.n_steps = {"prefill": 0, "decode": 0}
        self.on_launched = None  # hook after every step's launch (TP: enqueue the custom-AR error readback)
        # TP > 1 prefill as two micro-batches whose all-reduces overlap the other's compute
        # (K8SLLM_TP_OVERLAP=0: one batch, serial all-reduces)
        self.overlap = model.overlap_ok()
        self._last_ev = None  # end event of the last launched step (_chain_event)

    # --------------------------------------------------------------------- helpers
    @staticmethod
    def _micro_split(cu: np.ndarray, nd: int, min_rows: int = 4096) -> int:
        """First sequence of the second prefill micro-batch: the split nearest half the rows (0:
        no split - a mixed step, a single sequence, or fewer than ``min_rows`` rows, where the
        all-reduces are small and halving the GEMMs' M costs more than the overlap hides)."""
        S = len(cu) - 1
        if nd or S < 2 or cu[S] < min_rows:
            return 0
        k = int(np.argmin(np.abs(cu[1:S] - cu[S] / 2))) + 1
        if min(cu[k], cu[S] - cu[k]) < min_rows // 4:
            return 0  # too lopsided: the short half would leave the tile GEMM (TILE_MIN_M rows)
        return k

    def bucket_for(self, n: int) -> int:
        for b in self.buckets:
            if b >= n:
                return b
        raise ValueError(f"batch {n} exceeds max_num_seqs {self.B}")

    def _sample(self, logits: torch.Tensor, temp, topk, topp, out=None, pslot=None, gslot=None) -> torch.Tensor:
        # fresh numbers next step: the counter advances inside the sampling kernel (also in a graph)
        kw = {}
        if self.pen is not None:
            kw.update(penalties=self.pen, slots=pslot)
        if self.gd is not None:
            kw.update(guide=self.gd, gslots=gslot)
        return ops.sample(logits, temp, topk, topp, self.rng, out=out, advance=True, **kw)

    # --------------------------------------------------------------------- sampling penalties
    def penalty_enable(self) -> None:
        """Allocate the penalty state (``max_num_seqs`` slots) on first use.  Decode graphs
        captured without it sample without it: they are captured again, once, with the state and
        ``d_pslot`` as inputs (the in-flight step's tokens in ``d_out`` survive the capture)."""
        if self.pen is not None:
            return
        self.pen = ops.PenaltyState(self.B, self.model.cfg.vocab_size, self.device)
        self._pen_free = list(range(self.B - 1, -1, -1))
        if self.graphs:
            buckets = sorted(self.graphs)
            self.graphs, self.graphs_lora = {}, {}
            self.capture_graphs(buckets)

    def penalty_release(self, seq) -> None:
        """The sequence left the batch (finished, aborted, preempted): its slot is free.  A step
        still in flight may count one more token there; the next owner's reset runs after it."""
        slot = self._pen_slot.pop(getattr(seq, "seq_id", None), None)
        if slot is not None:
            self._pen_free.append(slot)

    def _penalty_slot(self, seq, take: bool = False) -> int:
        """The sequence's slot (-1: none).  ``take`` (a prefill chunk of a newly admitted or
        re-admitted sequence): a penalised sequence without a slot gets one, reset from its prompt
        and the tokens it generated before a preemption."""
        sid = getattr(seq, "seq_id", None)
        slot = self._pen_slot.get(sid, -1)
        p = seq.params
        if slot < 0 and take and sid is not None and p.has_penalties():
            if not self._pen_free:
                raise RuntimeError("no free penalty slot (more penalised sequences than max_num_seqs)")
            slot = self._pen_free.pop()
            self._pen_slot[sid] = slot
            self.pen.reset(slot, seq.prompt_ids, [t for t in seq.output_ids if t >= 0], p.repetition_penalty,
                           p.presence_penalty, p.frequency_penalty)
        return slot

    def _upload_pslot(self, seqs: list) -> None:
        """Decode rows -> slots, copied to ``d_pslot`` in front of the step only when it differs
        from what the device holds."""
        m = np.full(self.B, -1, dtype=np.int32)
        if self._pen_slot:
            m[: len(seqs)] = [self._pen_slot.get(s.seq_id, -1) for s in seqs]
        if np.array_equal(m, self._pslot_sent):
            return
        self._pslot_sent = m
        h = torch.from_numpy(m)
        self.d_pslot.copy_(h.pin_memory() if self.is_gpu else h, non_blocking=True)

    def penalty_stats(self) -> dict:
        return {"penalty_slots_in_use": len(self._pen_slot),
                "penalty_state_bytes": self.pen.nbytes if self.pen is not None else 0}

    # --------------------------------------------------------------------- constrained decoding
    def guide_enable(self, vocab_bytes, eos_ids, max_states: int) -> None:
        """Allocate the guide state on first use: ``max_num_seqs`` slots and ``max_num_seqs *
        max_states`` rows, so a guide always loads once unreferenced ones are evicted.  Decode
        graphs captured without it sample without it: they are captured again, once, with the state
        and ``d_gslot`` as inputs (the in-flight step's tokens in ``d_out`` survive the capture)."""
        if self.gd is not None:
            return
        self.gd = ops.GuideState(self.B, self.model.cfg.vocab_size, vocab_bytes, eos_ids, self.device,
                                 rows=self.B * int(max_states))
        self._gd_free = list(range(self.B - 1, -1, -1))
        if self.graphs:
            buckets = sorted(self.graphs)
            self.graphs, self.graphs_lora = {}, {}
            self.capture_graphs(buckets)

    def guide_release(self, seq) -> None:
        """The sequence left the batch (finished, aborted, preempted): its slot is free.  A step
        still in flight may advance the slot once more; the next owner's reset runs after it."""
        slot = self._gd_slot.pop(getattr(seq, "seq_id", None), None)
        if slot is not None:
            self.gd.release(slot)
            self._gd_free.append(slot)

    def _guide_slot(self, seq, take: bool = False) -> int:
        """The sequence's guide slot (-1: none).  ``take`` (a prefill chunk of a newly admitted or
        re-admitted sequence): a guided sequence without a slot gets one, reset to its guide's start
        state advanced over the tokens it generated before a preemption.  Unlike the penalty counts
        a guide cannot lose a token, so every one of those must be known: the engine reads the
        in-flight decode step back before it plans any prefill step (LLMEngine.step)."""
        sid = getattr(seq, "seq_id", None)
        slot = self._gd_slot.get(sid, -1)
        guide = getattr(seq, "guide", None)
        if slot < 0 and take and sid is not None and guide is not None:
            if any(t < 0 for t in seq.output_ids):
                raise RuntimeError("guide reset over a token still in flight")
            if not self._gd_free:
                raise RuntimeError("no free guide slot (more guided sequences than max_num_seqs)")
            slot = self._gd_free.pop()
            self._gd_slot[sid] = slot
            self.gd.reset(slot, guide, seq.output_ids)
        return slot

    def _upload_gslot(self, seqs: list) -> None:
        """Decode rows -> guide slots, copied to ``d_gslot`` in front of the step only when it
        differs from what the device holds."""
        m = np.full(self.B, -1, dtype=np.int32)
        if self._gd_slot:
            m[: len(seqs)] = [self._gd_slot.get(s.seq_id, -1) for s in seqs]
        if np.array_equal(m, self._gslot_sent):
            return
        self._gslot_sent = m
        h = torch.from_numpy(m)
        self.d_gslot.copy_(h.pin_memory() if self.is_gpu else h, non_blocking=True)

    def guide_stats(self) -> dict:
        g = self.gd
        return {"guide_enabled": g is not None, "guide_state_bytes": g.nbytes if g is not None else 0,
                "guides_resident": g.guides_resident if g is not None else 0,
                "guide_slots_in_use": len(self._gd_slot)}

    # --------------------------------------------------------------------- per-request LoRA
    def lora_setup(self) -> None:
        """The model holds adapters (CausalLM.enable_lora): allocate the decode rows' slot buffer."""
        if self.d_lslot is None:
            self.d_lslot = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
            self._lslot_sent = np.full(self.B, -1, dtype=np.int32)

    def lora_enable(self) -> None:
        """The first adapter request: from now on decode graphs exist in a second set, for steps
        with adapter rows (captured here for the buckets captured so far)."""
        if self.lora_on:
            return
        if self.d_lslot is None:
            raise RuntimeError("lora_enable before lora_setup")
        self.lora_on = True
        if self.graphs:
            self.capture_graphs(sorted(self.graphs), only_lora=True)

    def _upload_lslot(self, seqs: list) -> bool:
        """Decode rows -> adapter slots, copied to ``d_lslot`` in front of the step only when it
        differs from what the device holds.  False: no row of the step uses an adapter (nothing is
        uploaded - the step runs the plain path, which does not read the buffer)."""
        if not self.lora_on:
            return False
        sl = [getattr(s, "lora_slot", -1) for s in seqs]
        if max(sl, default=-1) < 0:
            return False
        m = np.full(self.B, -1, dtype=np.int32)
        m[: len(seqs)] = sl
        if not np.array_equal(m, self._lslot_sent):
            self._lslot_sent = m
            h = torch.from_numpy(m)
            self.d_lslot.copy_(h.pin_memory() if self.is_gpu else h, non_blocking=True)
        return True

    # --------------------------------------------------------------------- token log-probabilities
    def logprob_enable(self) -> None:
        """Allocate the logprob buffers on first use.  Decode graphs captured without the extra
        pass are captured again, once, with it and ``d_want`` as an input (the in-flight step's
        tokens in ``d_out`` survive the capture)."""
        if self.lp_on:
            return
        B, dev = self.B, self.device
        self.d_lp = torch.zeros(B, ops.LP_WIDTH, dtype=torch.int32, device=dev)
        self.d_want = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self._want_sent[:] = -1
        self.h_lp = [torch.zeros(B, ops.LP_WIDTH, dtype=torch.int32, pin_memory=self.is_gpu) for _ in range(2)]
        self.lp_on = True
        if self.graphs:
            buckets = sorted(self.graphs)
            self.graphs, self.graphs_lora = {}, {}
            self.capture_graphs(buckets)

    @staticmethod
    def _lp_want(seq) -> int:
        """What a sequence asks of ``ops.token_logprobs``: -1 nothing, else its ``top_logprobs``."""
        p = seq.params
        return int(p.top_logprobs) if getattr(p, "logprobs", False) else -1

    def _upload_want(self, seqs: list) -> Optional[list]:
        """Decode rows -> want, copied to ``d_want`` in front of the step only when it differs
        from what the device holds.  Returns the rows' wants, or None when no row asks."""
        want = [self._lp_want(s) for s in seqs]
        m = np.full(self.B, -1, dtype=np.int32)
        m[: len(seqs)] = want
        if not np.array_equal(m, self._want_sent):
            self._want_sent = m
            h = torch.from_numpy(m)
            self.d_want.copy_(h.pin_memory() if self.is_gpu else h, non_blocking=True)
        return want if max(want, default=-1) >= 0 else None

    @staticmethod
    def collect_logprobs(handle: "DecodeHandle") -> Optional[list]:
        """After :meth:`decode_collect`: per row of the step ``(lp, [(id, lp), ...])``
        (``ops.unpack_logprobs``) or None for a row that did not ask; None when no row did."""
        if handle.lp is None:
            return None
        rec = handle.lp[: handle.n].numpy()  # one conversion per step, not one per row
        lps = rec[:, : 1 + ops.LP_MAX_TOP].view(np.float32).tolist()
        ids = rec[:, 1 + ops.LP_MAX_TOP:].tolist()
        return [(f[0], [(i, v) for i, v in zip(t[:w], f[1:1 + w]) if i >= 0]) if w >= 0 else None
                for w, f, t in zip(handle.lp_want, lps, ids)]

    # --------------------------------------------------------------------- embedding requests
    def embed_enable(self) -> None:
        """The first embedding request: prefill steps stage ``edim`` from now on.  Decode steps and
        their graphs never carry an embedding row, so nothing is captured again."""
        self.embed_on = True

    @staticmethod
    def collect_embeddings(handle: "DecodeHandle") -> Optional[torch.Tensor]:
        """After :meth:`decode_collect`: the step's pooled rows, fp32 [>= rows, d_model] on the host
        (row r of the step is valid where that row was an embedding row), or None when it had none."""
        if handle.emb is not None and handle.event is not None:
            handle.event.synchronize()
        return handle.emb

    # --------------------------------------------------------------------- prefill
    def prefill(self, seqs: list[Sequence], decode: Optional[list] = None) -> list[int]:
        """One prefill (or mixed) step, synchronous: see :meth:`prefill_launch`."""
        return self.decode_collect(self.prefill_launch(seqs, decode))

    def _pf_stage(self, n: int) -> torch.Tensor:
        """Pinned int32 staging for one prefill step's inputs, alternating between two buffers
        (the previous step's copy may still be queued behind the step before it); grown on demand."""
        i = self._pf_i
        self._pf_i ^= 1
        buf = self._pf_bufs[i]
        if buf is None or buf.numel() < n:
            buf = torch.empty(max(n, 1 << 16) * 5 // 4, dtype=torch.int32, pin_memory=self.is_gpu)
            self._pf_bufs[i] = buf
        return buf

    def prefill_launch(self, seqs: list[Sequence], decode: Optional[list] = None) -> "DecodeHandle":
        """Enqueue each sequence's scheduled prefill chunk - tokens [num_computed, num_computed +
        chunk) of its prompt (+ any tokens generated before a preemption) - without waiting for it;
        the first num_computed tokens already have their KV in the cache (prefix-cache hits,
        earlier chunks) and are attended through the paged flash prefill.  ``decode`` (a mixed
        step): running sequences that also get their next token in this forward - their rows come
        first and attend through paged_decode.  The handle yields the sampled token of every decode
        row, then of every chunk (the first output token of the sequences whose prompt this step
        completes).  Every input goes over in ONE host-to-device copy from pinned memory, so a step
        can be enqueued while the previous one still runs (pipelined prefill)."""
        dev = self.device
        decode = decode or []
        nd = len(decode)
        starts = [s.num_computed for s in seqs]
        lens = [s.chunk or (s.num_tokens - c) for s, c in zip(seqs, starts)]
        T = nd + sum(lens)
        rows = list(decode) + list(seqs)
        R = len(rows)
        cu = np.zeros(len(seqs) + 1, dtype=np.int32)
        cu[1:] = np.cumsum(lens)
        qs, st = ops.prefill_qblocks(cu.tolist(), ctx_starts=starts)
        nq = len(qs)
        paged = any(starts)
        W = max(len(s.block_table) for s in seqs) if paged else 0
        Wd = max(len(q.block_table) for q in decode) if nd else 0
        # TP > 1: two micro-batches of whole sequences, so one's row-parallel all-reduces overlap
        # the other's compute (models/llama.py _prefill_overlap); their own cu_seqlens / q-block
        # schedules / logits rows ride in the same staging copy
        kA = self._micro_split(cu, nd) if self.overlap else 0
        mb = None
        if kA:
            cuA, cuB = cu[: kA + 1], cu[kA:] - cu[kA]
            mb = (ops.prefill_qblocks(cuA.tolist(), ctx_starts=starts[:kA]),
                  ops.prefill_qblocks(cuB.tolist(), ctx_starts=starts[kA:]))
        # layout of the staging buffer (int32 words; the float sampling parameters bit-cast)
        sizes = dict(ids=T, pos=T, slots=T, cu=len(seqs) + 1, qs=nq, st=nq, lidx=R, temp=R, topk=R, topp=R,
                     cst=len(seqs) if paged else 0, bt=len(seqs) * W, dbt=nd * Wd, dlen=nd,
                     mcu=len(seqs) + 2 if kA else 0, mqs=nq if kA else 0, mst=nq if kA else 0,
                     mlidx=len(seqs) if kA else 0, pslot=R if self.pen is not None else 0,
                     want=R if self.lp_on else 0, gslot=R if self.gd is not None else 0,
                     lslot=T if self.lora_on and any(getattr(s, "lora_slot", -1) >= 0 for s in rows) else 0,
                     edim=R if self.embed_on else 0)
        off, o = {}, 0
        for k, n in sizes.items():
            off[k] = o
            o += n
        buf = self._pf_stage(o)
        h = buf.numpy()
        v = {k: h[off[k]:off[k] + n] for k, n in sizes.items()}
        ids, pos, slots = v["ids"], v["pos"], v["slots"]
        for i, q in enumerate(decode):  # the token being fed is the last generated one
            p = q.num_tokens - 1
            ids[i] = q.last_token
            pos[i] = p
            slots[i] = q.block_table[p // BLOCK_SIZE] * BLOCK_SIZE + p % BLOCK_SIZE
        o = nd
        for s, c, n in zip(seqs, starts, lens):
            ch = getattr(s, "chunk_ids", None)  # TP worker views carry just the chunk
            ids[o:o + n] = ch if ch is not None else s.all_ids[c:c + n]
            p = np.arange(c, c + n, dtype=np.int32)
            pos[o:o + n] = p
            bt = np.asarray(s.block_table, dtype=np.int32)
            slots[o:o + n] = bt[p // BLOCK_SIZE] * BLOCK_SIZE + p % BLOCK_SIZE
            o += n
        v["cu"][:] = cu
        v["qs"][:] = qs
        v["st"][:] = st
        v["lidx"][:nd] = np.arange(nd, dtype=np.int32)
        v["lidx"][nd:] = nd + cu[1:] - 1
        v["temp"].view(np.float32)[:] = [s.params.temperature for s in rows]
        v["topk"][:] = [s.params.top_k for s in rows]
        v["topp"].view(np.float32)[:] = [s.params.top_p for s in rows]
        if self.pen is not None:
            # a chunk short of its prompt's end samples a token nobody keeps: it must not be counted
            v["pslot"][:nd] = [self._penalty_slot(q) for q in decode]
            for i, (s, c, n) in enumerate(zip(seqs, starts, lens)):
                slot = self._penalty_slot(s, take=True)
                v["pslot"][nd + i] = slot if c + n >= s.num_tokens else -1
        if self.gd is not None:
            # a chunk short of its prompt's end samples a token nobody keeps: it must not advance the state
            v["gslot"][:nd] = [self._guide_slot(q) for q in decode]
            for i, (s, c, n) in enumerate(zip(seqs, starts, lens)):
                slot = self._guide_slot(s, take=True)
                v["gslot"][nd + i] = slot if c + n >= s.num_tokens else -1
        if sizes["lslot"]:  # one adapter slot per token row of the step
            v["lslot"][:nd] = [getattr(q, "lora_slot", -1) for q in decode]
            o = nd
            for s, n in zip(seqs, lens):
                v["lslot"][o:o + n] = getattr(s, "lora_slot", -1)
                o += n
        lp_want = None
        if self.lp_on:
            # a chunk short of its prompt's end samples a token nobody keeps: no logprobs for it
            v["want"][:nd] = [self._lp_want(q) for q in decode]
            v["want"][nd:] = [self._lp_want(s) if c + n >= s.num_tokens else -1
                              for s, c, n in zip(seqs, starts, lens)]
            if int(v["want"].max()) >= 0:
                lp_want = v["want"].tolist()
        has_emb, want_logits = False, True
        if self.embed_on:
            # the row of a chunk that reaches the end of an embedding sequence's prompt is pooled; the
            # head and the sampler run unless no row of the step needs a token
            v["edim"][:nd] = 0
            v["edim"][nd:] = [getattr(s, "embed_dim", 0) if c + n >= s.num_tokens else 0
                              for s, c, n in zip(seqs, starts, lens)]
            has_emb = bool(v["edim"].any())
            want_logits = bool(nd) or not all(getattr(s, "embed_dim", 0) for s in seqs)
        if paged:
            v["cst"][:] = starts
            bt2 = v["bt"].reshape(len(seqs), W)
            bt2[:] = 0
            for i, s in enumerate(seqs):
                bt2[i, : len(s.block_table)] = s.block_table
        if nd:
            dbt = v["dbt"].reshape(nd, Wd)
            dbt[:] = 0
            for i, q in enumerate(decode):
                dbt[i, : len(q.block_table)] = q.block_table
            v["dlen"][:] = [q.num_tokens for q in decode]
        if kA:
            v["mcu"][: kA + 1] = cuA
            v["mcu"][kA + 1:] = cuB
            nqA = len(mb[0][0])
            v["mqs"][:nqA], v["mst"][:nqA] = mb[0]
            v["mqs"][nqA:], v["mst"][nqA:] = mb[1]
            v["mlidx"][:kA] = cuA[1:] - 1
            v["mlidx"][kA:] = cuB[1:] - 1
        d = buf[: sum(sizes.values())].to(dev, non_blocking=True)
        dv = {k: d[off[k]:off[k] + n] for k, n in sizes.items()}
        meta = AttnMeta(is_prefill=True, positions=dv["pos"], slot_mapping=dv["slots"], cu_seqlens=dv["cu"],
                        qb_seq=dv["qs"], qb_start=dv["st"], logits_idx=dv["lidx"].long())
        if sizes["lslot"]:
            meta.lora_slot = dv["lslot"]
        if has_emb:
            meta.pool_dim = dv["edim"]
            if self.is_gpu:  # (the CPU path hands the step's own tensor to the handle)
                # rows that are no embedding rows keep whatever the buffer held: nobody reads them
                if self._d_emb is None or self._d_emb.shape[0] < R:
                    self._d_emb = torch.zeros(max(R, 2 * self.B), self.model.cfg.d_model, dtype=torch.float32,
                                              device=dev)
                meta.pooled = self._d_emb[:R]
        meta.want_logits = want_logits
        if paged:
            meta.ctx_start = dv["cst"]
            meta.block_tables = dv["bt"].view(len(seqs), W)
        if kA:
            TA, S_ = int(cu[kA]), len(seqs)
            parts = []
            for (r0, r1), (s0, s1), (q0, q1) in ((((0, TA), (0, kA), (0, nqA))),
                                                 ((TA, T), (kA, S_), (nqA, nq))):
                m = AttnMeta(is_prefill=True, positions=dv["pos"][r0:r1], slot_mapping=dv["slots"][r0:r1],
                             cu_seqlens=dv["mcu"][s0 + (s0 > 0): s1 + 1 + (s0 > 0)], qb_seq=dv["mqs"][q0:q1],
                             qb_start=dv["mst"][q0:q1], logits_idx=dv["mlidx"][s0:s1].long())
                if paged:
                    m.ctx_start = dv["cst"][s0:s1]
                    m.block_tables = dv["bt"].view(S_, W)[s0:s1]
                parts.append(m)
            meta.micro = (parts[0], parts[1], TA)
            self.n_steps["overlapped"] = self.n_steps.get("overlapped", 0) + 1
        if nd:
            meta.num_decode = nd
            meta.dec_block_tables = dv["dbt"].view(nd, Wd)
            meta.dec_seq_lens = dv["dlen"]
            meta.decode_ws = self.decode_ws
            self.n_steps["mixed"] = self.n_steps.get("mixed", 0) + 1
        # tokens attended from the paged cache instead of recomputed (prefix hits + earlier chunks)
        self.n_steps["prefill_context_tokens"] = self.n_steps.get("prefill_context_tokens", 0) + sum(starts)
        self.n_steps["prefill_tokens"] = self.n_steps.get("prefill_tokens", 0) + T
        logits = self.model.forward(dv["ids"], meta, self.kv)
        tok = lp = None
        if want_logits:  # else an embedding-only step: no head (forward), no sampler, no tokens
            tok = self._sample(logits, dv["temp"].view(torch.float32), dv["topk"], dv["topp"].view(torch.float32),
                               pslot=dv["pslot"], gslot=dv["gslot"])
            lp = ops.token_logprobs(logits[:R], tok, dv["want"]) if lp_want is not None else None
        emb = meta.pooled if has_emb else None
        self.n_steps["prefill"] += 1
        if self.on_launched is not None:  # TP: the custom-AR error flag, read back with the tokens
            self.on_launched()
        if not self.is_gpu:
            return DecodeHandle(R, None, tok[:R].tolist() if tok is not None else None, lp=lp, lp_want=lp_want,
                                emb=emb)
        j = self._pf_oi
        self._pf_oi ^= 1  # two in flight at most: step N+1 is launched before step N is read back
        out = None
        if tok is not None:
            if self._pf_out[j] is None or self._pf_out[j].numel() < R:
                self._pf_out[j] = torch.empty(max(R, 2 * self.B), dtype=torch.int32, pin_memory=True)
            out = self._pf_out[j]
            out[:R].copy_(tok[:R], non_blocking=True)
        h_emb = None
        if emb is not None:
            if self._pf_emb[j] is None or self._pf_emb[j].shape[0] < R:
                self._pf_emb[j] = torch.empty(max(R, 2 * self.B), emb.shape[1], dtype=torch.float32, pin_memory=True)
            h_emb = self._pf_emb[j]
            h_emb[:R].copy_(emb, non_blocking=True)
        h_lp = None
        if lp is not None:
            if self._pf_lp[j] is None or self._pf_lp[j].shape[0] < R:
                self._pf_lp[j] = torch.empty(max(R, 2 * self.B), ops.LP_WIDTH, dtype=torch.int32, pin_memory=True)
            h_lp = self._pf_lp[j]
            h_lp[:R].copy_(lp, non_blocking=True)
        ev, _ = self._chain_event()
        return DecodeHandle(R, ev, out, lp=h_lp, lp_want=lp_want, emb=h_emb)

    # --------------------------------------------------------------------- decode
    def _decode_body(self, b: int, lora: bool = False) -> None:
        # pipelined decode: a row whose input is the token sampled by the previous step (still in
        # flight when this step was enqueued) takes it from d_out on the device (d_src = its row
        # there); other rows take the host-provided id - resolved by the model's first kernel
        meta = AttnMeta(is_prefill=False, positions=self.d_pos[:b], slot_mapping=self.d_slots[:b],
                        block_tables=self.d_bt[:b], seq_lens=self.d_lens[:b], decode_ws=self.decode_ws,
                        dec_src=self.d_src[:b], dec_prev=self.d_out, lora_slot=self.d_lslot[:b] if lora else None)
        logits = self.model.forward(self.d_ids[:b], meta, self.kv)
        self._sample(logits, self.d_temp[:b], self.d_topk[:b], self.d_topp[:b], out=self.d_out[:b],
                     pslot=self.d_pslot[:b], gslot=self.d_gslot[:b])
        if self.lp_on:  # after the sampler on the stream: it reads the tokens just drawn
            ops.token_logprobs(logits, self.d_out[:b], self.d_want[:b], out=self.d_lp[:b])

    def capture_graphs(self, buckets: Optional[list[int]] = None, only_lora: bool = False) -> None:
        """Capture the decode graphs of ``buckets`` (all by default): the plain set and, once an
        adapter request was seen (lora_on), the set for steps with adapter rows; ``only_lora``: the
        latter alone (lora_enable)."""
        if not (self.is_gpu and self.cfg.use_graphs):
            return
        kinds = ([] if only_lora else [False]) + ([True] if self.lora_on else [])
        torch.cuda.synchronize()
        # replays must not disturb real sequences: capture with empty rows (len 0, no cache write)
        self.d_lens.zero_()
        self.d_slots.fill_(-1)
        self.d_pslot.fill_(-1)  # ... and count nothing; the next decode step uploads its rows' slots again
        self._pslot_sent[:] = -1
        self.d_gslot.fill_(-1)  # ... and advance no guide
        self._gslot_sent[:] = -1
        if self.lp_on:  # ... and compute no logprobs
            self.d_want.fill_(-1)
            self._want_sent[:] = -1
        if self.d_lslot is not None:  # ... and apply no adapter
            self.d_lslot.fill_(-1)
            self._lslot_sent[:] = -1
        rng_state, out_state = self.rng.clone(), self.d_out.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for lora in kinds:
                for _ in range(2):
                    self._decode_body(self.B, lora)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph_pool = torch.cuda.graph_pool_handle()
        for b in sorted(buckets or self.buckets, reverse=True):
            n_el = _Staging.prefix(self.B, self.max_blocks_per_seq, b)
            for lora in kinds:
                gs = []
                for st in (self.stage if self.graph_h2d else [None]):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, pool=self.graph_pool):
                        if st is not None:
                            self.d_all[:n_el].copy_(st.h_all[:n_el], non_blocking=True)
                        self._decode_body(b, lora)
                    gs.append(g)
                (self.graphs_lora if lora else self.graphs)[b] = gs
        torch.cuda.synchronize()
        self.rng.copy_(rng_state)
        self.d_out.copy_(out_state)

    def decode(self, seqs: list, src_rows: Optional[list] = None, publish=None) -> list[int]:
        """One decode step, synchronous: the sampled token per sequence."""
        return self.decode_collect(self.decode_launch(seqs, src_rows, publish))

    def decode_launch(self, seqs: list, src_rows: Optional[list] = None, publish=None) -> "DecodeHandle":
        """Enqueue one decode step without waiting for it.  ``src_rows[i] >= 0``: sequence i's input
        token is the one the previous (possibly still running) step sampled in that row; else its
        ``last_token``.  Positions come from ``num_tokens``, so a sequence carrying a not yet
        resolved token from the in-flight step is already one position further.  ``publish``
        (TP leader): called with the raw step message (parallel/step_bus.py) after staging and
        before the launch, so the workers replay the same step."""
        n = len(seqs)
        b = self.bucket_for(n) if self.graphs else n
        st = self.stage[self._stage_i]
        self._stage_i ^= 1
        ids, pos_a, slots, lens, src = st.n_ids, st.n_pos, st.n_slots, st.n_lens, st.n_src
        temp, topk, topp, bt_a = st.n_temp, st.n_topk, st.n_topp, st.n_bt
        bt_a[:b] = 0
        for i, s in enumerate(seqs):
            pos = s.num_tokens - 1  # position of the token being fed (the last generated one)
            bt = s.block_table
            r = src_rows[i] if src_rows is not None else -1
            src[i] = r
            ids[i] = s.last_token if r < 0 else 0
            pos_a[i] = pos
            slots[i] = bt[pos // BLOCK_SIZE] * BLOCK_SIZE + pos % BLOCK_SIZE
            lens[i] = pos + 1
            bt_a[i, : len(bt)] = bt
            p = s.params
            temp[i] = p.temperature
            topk[i] = p.top_k
            topp[i] = p.top_p
        if b > n:
            ids[n:b] = 0
            src[n:b] = -1
            pos_a[n:b] = 0
            slots[n:b] = -1
            lens[n:b] = 0
            temp[n:b] = 0
            topk[n:b] = 0
            topp[n:b] = 1
        n_el = _Staging.prefix(self.B, self.max_blocks_per_seq, b)  # the per-row fields + b block-table rows
        if self.pen is not None:
            self._upload_pslot(seqs)
        if self.gd is not None:
            self._upload_gslot(seqs)
        lp_want = self._upload_want(seqs) if self.lp_on else None
        lora = self._upload_lslot(seqs)
        if publish is not None:
            publish(st.message(n, b, n_el))
        return self._launch_staged(st, n, b, n_el, lp_want, lora)

    def decode_launch_raw(self, n: int, b: int, n_el: int, words: np.ndarray) -> "DecodeHandle":
        """TP worker: launch the decode step the leader staged (its raw staging words)."""
        st = self.stage[self._stage_i]
        self._stage_i ^= 1
        st.raw[:n_el] = words
        return self._launch_staged(st, n, b, n_el)

    def _launch_staged(self, st: "_Staging", n: int, b: int, n_el: int,
                       lp_want: Optional[list] = None, lora: bool = False) -> "DecodeHandle":
        """``lp_want`` (logprobs enabled and some row of the step asks): the rows' wants - their
        records are read back beside the tokens.  ``lora``: some row of the step uses an adapter -
        the graph set captured with ``d_lslot`` as an input."""
        gs = (self.graphs_lora if lora else self.graphs).get(b)
        if gs is not None and self.graph_h2d:
            gs[st.idx].replay()  # its first node copies this staging buffer (n_el = the bucket's prefix)
        else:
            self.d_all[:n_el].copy_(st.h_all[:n_el], non_blocking=True)
            if gs is not None:
                gs[0].replay()
            else:
                self._decode_body(b, lora)
        self.n_steps["decode"] += 1
        if self.on_launched is not None:
            self.on_launched()
        if not self.is_gpu:
            return DecodeHandle(n, None, self.d_out[:n].tolist(),
                                lp=self.d_lp[:n].clone() if lp_want is not None else None, lp_want=lp_want)
        h = self.h_out[self._out_i]
        h_lp = self.h_lp[self._out_i] if lp_want is not None else None
        self._out_i ^= 1
        h[:n].copy_(self.d_out[:n], non_blocking=True)
        if h_lp is not None:
            h_lp[:n].copy_(self.d_lp[:n], non_blocking=True)
        ev, prev = self._chain_event()
        return DecodeHandle(n, ev, h, prev, lp=h_lp, lp_want=lp_want)

    def _chain_event(self) -> tuple:
        """Record the end-of-step event (timing-enabled) and return it with the previous launched
        step's event IF that step was still running when this one was enqueued: the GPU then went
        from one step straight into the next, so the elapsed time between the two events is this
        step's GPU time (no host stall inside it) - the decode step-time samples of the admission
        model (EngineService.tpot).  Otherwise the previous event is dropped (None)."""
        prev = self._last_ev
        busy = prev is not None and not prev.query()
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self._last_ev = ev
        return ev, (prev if busy else None)

    @staticmethod
    def decode_collect(handle: "DecodeHandle") -> list[int]:
        if handle.event is not None:
            handle.event.synchronize()
        if handle.out is None:  # an embedding-only prefill step drew no tokens
            return [-1] * handle.n
        return handle.out if handle.event is None else handle.out[: handle.n].tolist()

    def kv_stats(self) -> dict:
        """The paged cache as allocated: its encoding, blocks and true bytes (codes + scales for fp8)."""
        return {"kv_cache_dtype": self.kv_cache_dtype, "kv_cache_bytes": self.kv_cache_bytes,
                "kv_blocks": self.num_blocks, "block_size": BLOCK_SIZE}

    def memory_report(self) -> dict:
        return {**self.kv_stats(), "max_model_len": self.max_len, "graph_buckets": sorted(self.graphs),
                "penalty_state_bytes": self.penalty_stats()["penalty_state_bytes"],
                "guide_state_bytes": self.guide_stats()["guide_state_bytes"]}


class _Staging:
    """Pinned host buffer for one decode step's inputs, with numpy views for cheap writes.

    One int32 buffer holds every field - ids, src, pos, slots, lens, top_k, temperature and top_p
    ([B] each; the two float fields bit-cast) followed by the block tables [B, max_blocks] - so the
    step's inputs reach the device in ONE copy of the per-row fields plus the live block-table rows
    (nine separate small copies were nine blit kernels of ~4.6 us each in front of every decode
    graph replay)."""

    NFIELDS = 8

    @staticmethod
    def size(B: int, max_blocks: int) -> int:
        return _Staging.NFIELDS * B + B * max_blocks

    @staticmethod
    def prefix(B: int, max_blocks: int, b: int) -> int:
        return _Staging.NFIELDS * B + b * max_blocks

    @staticmethod
    def views(buf, B: int, max_blocks: int) -> tuple:
        """(ids, src, pos, slots, lens, topk, temp, topp, bt) views of a buffer (torch or numpy)."""
        f = [buf[i * B:(i + 1) * B] for i in range(_Staging.NFIELDS)]
        as_f32 = (lambda a: a.view(torch.float32)) if isinstance(buf, torch.Tensor) else (lambda a: a.view(np.float32))
        f[6], f[7] = as_f32(f[6]), as_f32(f[7])
        bt = buf[_Staging.NFIELDS * B:_Staging.size(B, max_blocks)]
        bt = bt.view(B, max_blocks) if isinstance(buf, torch.Tensor) else bt.reshape(B, max_blocks)
        return (*f, bt)

    def __init__(self, B: int, max_blocks: int, pin: bool, idx: int = 0):
        from ..parallel.step_bus import DECODE_HDR, KIND_DECODE

        self.idx = idx
        # DECODE_HDR leading words hold the step-bus header, so a TP leader publishes
        # full[:DECODE_HDR + n_el] without a copy (parallel/step_bus.py)
        self.h_full = torch.zeros(DECODE_HDR + self.size(B, max_blocks), dtype=torch.int32, pin_memory=pin)
        self.h_all = self.h_full[DECODE_HDR:]
        self.full = self.h_full.numpy()
        self.full[0] = KIND_DECODE
        self.raw = self.full[DECODE_HDR:]
        (self.n_ids, self.n_src, self.n_pos, self.n_slots, self.n_lens, self.n_topk, self.n_temp, self.n_topp,
         self.n_bt) = self.views(self.raw, B, max_blocks)

    def message(self, n: int, b: int, n_el: int) -> np.ndarray:
        from ..parallel.step_bus import DECODE_HDR

        self.full[1:4] = (n, b, n_el)
        return self.full[:DECODE_HDR + n_el]


@dataclass
class DecodeHandle:
    n: int
    event: object  # torch.cuda.Event, None on the CPU
    out: object  # pinned host tensor (GPU) or the token list (CPU)
    prev_event: object = None  # the back-to-back predecessor's end event (ModelRunner._chain_event)
    lp: object = None  # the step's packed logprob records (pinned on the GPU), None when no row asked
    lp_want: Optional[list] = None  # with lp: per row what it asked (-1: nothing, its record is stale)
    emb: object = None  # a prefill step's pooled rows, fp32 [>= n, d_model] (pinned on the GPU), None without embedding rows

    def gpu_ms(self) -> Optional[float]:
        """This step's GPU time (after the event completed), or None when not measurable."""
        if self.prev_event is None or self.event is None:
            return None
        return float(self.prev_event.elapsed_time(self.event))


def kv_blocks_for(cfg_layers: int, hkv: int, D: int, gb: float) -> int:
    per_block = 2 * cfg_layers * hkv * D * BLOCK_SIZE * 2
    return int(math.floor(gb * (1 << 30) / per_block))
