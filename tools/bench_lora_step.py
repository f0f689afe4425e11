#!/usr/bin/env python
"""What per-request LoRA adapters cost a decode step (profiles/r25/README.md, profiles/r26/README.md).

    python tools/bench_lora_step.py --mode step [--adapters 4 --rank 16 --rows 64,1 --ctx 1750 --targets all]
    python tools/bench_lora_step.py --mode kernels

``step``: one Llama-3-8B engine (graphs, pipelined decode), ``--adapters`` random rank-``--rank``
adapters on q, k, v, o and down (``--targets attn_down``, the default) or on all seven projections
(``--targets all``: gate and up too, which allocates the gate_up arena) written to a temporary
directory and configured (0: none configured - this mode then also runs on a tree without the
feature), waves of ``rows`` requests of about ``ctx``
prompt tokens and ``--tokens`` generated ones; GPU time of the back-to-back ``rows``-row decode steps
from the engine's own events (``LLMEngine.step_samples``), the first ten of a wave dropped.  Phases,
each one wave after an unreported warm-up wave: ``base`` (no row names an adapter; before the first
adapter request), then - with adapters - ``one_row`` (1 row on adapter 0), ``all_one`` (every row on
adapter 0), ``spread`` (rows cycling over all adapters) and ``base_after``.
``kernels``: lora_shrink + lora_expand alone at the 8B shapes (qkv 6144 x 4096 at capacity 192, o 4096
x 4096 and down 4096 x 14336 at capacity 64, gate_up 28672 x 4096 at capacity 128), 64 rows and 1 row,
1 and 4 adapters present, 20 calls per captured graph, the median of 5 timings of 20 replays; then
the gate_up decode GEMM (28672 x 4096, SwiGLU epilogue) alone without and with the pre-activation
delta, every row on an adapter, timed the same way."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _write_adapters(n: int, rank: int, cfg, root: str, targets: str = "attn_down") -> dict:
    from k8s_llm_monitor_amd.models.checkpoint import LoraAdapter, save_lora

    D, d = cfg.head_dim, cfg.d_model
    shapes = {"q_proj": (cfg.n_heads * D, d), "k_proj": (cfg.n_kv_heads * D, d), "v_proj": (cfg.n_kv_heads * D, d),
              "o_proj": (d, cfg.n_heads * D), "down_proj": (d, cfg.ffn_dim)}
    if targets == "all":
        shapes.update({"gate_proj": (cfg.ffn_dim, d), "up_proj": (cfg.ffn_dim, d)})
    out = {}
    for a in range(n):
        g = torch.Generator().manual_seed(100 + a)
        t = {(layer, m): ((torch.randn(rank, i, generator=g) * 0.01).to(torch.bfloat16),
                          (torch.randn(o, rank, generator=g) * 0.01).to(torch.bfloat16))
             for layer in range(cfg.n_layers) for m, (o, i) in shapes.items()}
        ad = LoraAdapter(r=rank, lora_alpha=2.0 * rank, target_modules=tuple(sorted(shapes)), tensors=t, name=f"ad{a}")
        out[ad.name] = str(save_lora(ad, os.path.join(root, ad.name)))
    return out


def step_mode(a) -> None:
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from k8s_llm_monitor_amd.models.config import get_config

    rows_list = [int(r) for r in a.rows.split(",")]
    kw = {}
    with tempfile.TemporaryDirectory() as root:
        if a.adapters:
            kw = {"lora_adapters": _write_adapters(a.adapters, a.rank, get_config(a.model), root, a.targets),
                  "lora_max_rank": a.max_rank}
        eng = LLMEngine(EngineConfig(model=a.model, max_num_seqs=max(rows_list), max_model_len=4096, kv_cache_gb=48.0,
                                     seed=1, **kw), device="cuda")
    eng.warmup()
    names = sorted(getattr(eng, "adapters", {}) or {})
    st = eng.stats()
    print(json.dumps({"adapters": len(names), "rank": a.rank, "targets": a.targets, "lora_bytes": st.get("lora_bytes"),
                      "resident_weight_bytes": st.get("resident_weight_bytes")}), flush=True)
    g = torch.Generator().manual_seed(5)

    def wave(rows, prompts, pick, label):
        seqs = []
        for i, p in enumerate(prompts):
            sp = SamplingParams(max_tokens=a.tokens, temperature=0.0, ignore_eos=True)
            if pick(i) is not None:
                sp.adapter = pick(i)
            seqs.append(eng.add_request(p, sp))
        eng.step_samples.clear()
        while eng.has_work():
            eng.step()
        ms = sorted(m for (n, m, *_) in list(eng.step_samples)[10:] if n == rows)
        if label is not None and ms:
            print(json.dumps({"phase": label, "rows": rows, "steps": len(ms), "median_step_ms": round(statistics.median(ms), 4),
                              "p10": round(ms[len(ms) // 10], 4), "p90": round(ms[len(ms) * 9 // 10], 4),
                              "lora_enabled": eng.stats().get("lora_enabled")}), flush=True)

    for rows in rows_list:
        prompts = [torch.randint(100, 120000, (a.ctx + (i * 37) % 100,), generator=g).tolist() for i in range(rows)]
        wave(rows, prompts, lambda i: None, None)
        wave(rows, prompts, lambda i: None, "base")
        if names:
            wave(rows, prompts, lambda i: names[0] if i == 0 else None, "one_row")
            wave(rows, prompts, lambda i: names[0], "all_one")
            wave(rows, prompts, lambda i: names[i % len(names)], "spread")
            wave(rows, prompts, lambda i: None, "base_after")


def kernels_mode(a) -> None:
    from k8s_llm_monitor_amd import ops

    dev = "cuda"
    shapes = {"wqkv": (6144, 4096, 192), "wo": (4096, 4096, 64), "w2": (4096, 14336, 64), "w13": (28672, 4096, 128)}
    st = ops.LoraState(4, 1, shapes, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for p, (N, K, R) in shapes.items():
        st.A[p].copy_((torch.randn(st.A[p].shape, device=dev, generator=g) * 0.01).to(torch.bfloat16))
        st.B[p].copy_((torch.randn(st.B[p].shape, device=dev, generator=g) * 0.01).to(torch.bfloat16))
    st.scaling.fill_(2.0)
    def timed(fn):
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(20):
                fn()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / 400)
        return round(statistics.median(ts), 2)

    # the gate_up decode GEMM alone, without and with the delta (every row on an adapter)
    F, K = 14336, 4096
    w13 = ops.pack_skinny(ops.interleave_gate_up8((torch.randn(2 * F, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)))
    for M in (64, 1):
        x = ops.pack_activation(torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16))
        act = ops.packed_empty(M, F, torch.bfloat16, dev)
        delta = torch.randn(M * 2 * F, device=dev, generator=g)
        slot = torch.zeros(M, dtype=torch.int32, device=dev)
        for _ in range(2):  # twice, alternating: the spread of the same launch beside the difference
            for label, kw in (("plain", {}), ("delta", dict(delta=delta, delta_slot=slot, delta_slots=4))):
                us = timed(lambda: ops.dec_gemm(x, w13, 2, M, out=act, **kw))
                print(json.dumps({"gemm": "gate_up", "N": 2 * F, "K": K, "rows": M, "form": label, "us": us}), flush=True)
    for M in (64, 1):
        for present in (1, 4):
            slot = torch.tensor([i % present for i in range(M)], dtype=torch.int32, device=dev)
            for p, (N, K, R) in shapes.items():
                x = ops.pack_activation(torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16))
                ws = torch.zeros(2 * M * N, device=dev)
                us = timed(lambda: ops.lora_slab(st, 0, p, x, M, ws, 1, slot))
                print(json.dumps({"proj": p, "N": N, "K": K, "R": R, "rows": M, "adapters_present": present,
                                  "S": ops.lora_shrink_plan(K), "us_per_pair": us}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="step", choices=["step", "kernels"])
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--adapters", type=int, default=4)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--max-rank", type=int, default=64)
    ap.add_argument("--rows", default="64,1")
    ap.add_argument("--ctx", type=int, default=1750)
    ap.add_argument("--tokens", type=int, default=96)
    ap.add_argument("--targets", default="attn_down", choices=["attn_down", "all"])
    a = ap.parse_args()
    (step_mode if a.mode == "step" else kernels_mode)(a)


if __name__ == "__main__":
    main()
