#!/usr/bin/env python
"""What ``llm.prefill_weights: fp8`` costs and saves, end to end, in ONE process on one box: for
each weight mode - ``bf16``, ``fp8`` (decode_weights: fp8, codes beside the bf16 copy) and
``fp8only`` (+ prefill_weights: fp8, the bf16 copy released), and the same pair over MXFP4
(``mxfp4``, ``mxfp4only``) - build the engine, warm it up and
record

  * ``resident_weight_bytes`` (engine.stats()) and the GPU allocator's figures after warm-up,
  * the time of one prefill forward of ``--prefill-tokens`` tokens (median of ``--reps``, GPU events),
  * the median decode step at ``--rows`` rows and ~``--ctx``-token contexts (LLMEngine.step_samples).

The modes run in turn, ``--rounds`` times over (a mode's engine is freed before the next is built),
so every mode is measured more than once and next to the others.  One JSON line per mode and round.

    python tools/bench_prefill_f8.py [--model llama-3-8b] [--modes bf16,fp8,fp8only] [--rounds 2]
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

MODES = {"bf16": {}, "fp8": {"decode_weights": "fp8"}, "fp8only": {"decode_weights": "fp8", "prefill_weights": "fp8"},
         "mxfp4": {"decode_weights": "mxfp4"}, "mxfp4only": {"decode_weights": "mxfp4", "prefill_weights": "mxfp4"}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--layers", type=int, default=0, help="override the model's layer count (0 = all)")
    ap.add_argument("--modes", default="bf16,fp8,fp8only")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--prefill-tokens", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--ctx", type=int, default=1000)
    ap.add_argument("--tokens", type=int, default=48)
    ap.add_argument("--kv-cache-gb", type=float, default=16.0)
    a = ap.parse_args()
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from k8s_llm_monitor_amd.models import AttnMeta

    g = torch.Generator().manual_seed(5)
    n = a.prefill_tokens
    ids = torch.randint(100, 30000, (n,), generator=g, dtype=torch.int32).cuda()
    prompts = [torch.randint(100, 30000, (a.ctx + (i * 37) % 100,), generator=g).tolist() for i in range(a.rows)]
    sp = SamplingParams(max_tokens=a.tokens, temperature=0.0, ignore_eos=True)
    for rnd in range(a.rounds):
        for mode in a.modes.split(","):
            torch.cuda.reset_peak_memory_stats()
            eng = LLMEngine(EngineConfig(model=a.model, max_num_seqs=a.rows, max_model_len=4096,
                                         kv_cache_gb=a.kv_cache_gb, seed=1, prefix_caching=False,
                                         model_overrides={"n_layers": a.layers} if a.layers else {}, **MODES[mode]),
                            device="cuda")
            build_peak = torch.cuda.max_memory_allocated()
            eng.warmup()
            torch.cuda.synchronize()
            st = eng.stats()
            alloc, kv_bytes = torch.cuda.memory_allocated(), st.get("kv_cache_bytes", 0)
            meta = AttnMeta(is_prefill=True, positions=torch.arange(n, dtype=torch.int32, device="cuda"),
                            slot_mapping=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                            cu_seqlens=torch.tensor([0, n], dtype=torch.int32, device="cuda"),
                            logits_idx=torch.tensor([n - 1], device="cuda"))
            ms = []
            with torch.no_grad():
                for _ in range(a.reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    eng.model.forward(ids, meta, None)
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
            eng.step_samples.clear()
            eng.generate(prompts, sp)
            dec = [m for (r, m, _) in eng.step_samples if r == a.rows]
            print(json.dumps({"mode": mode, "round": rnd, "model": st["model"], "layers": len(eng.model.layers),
                              "resident_weight_bytes": st["resident_weight_bytes"],
                              "allocated_after_warmup_bytes": alloc, "kv_cache_bytes": kv_bytes,
                              "allocated_minus_kv_bytes": alloc - kv_bytes, "peak_during_build_bytes": build_peak,
                              "prefill_encodings": st["prefill_encodings"], "decode_encodings": st["decode_encodings"],
                              "prefill_tokens": n, "prefill_ms_median": round(statistics.median(ms[1:]), 3),
                              "prefill_ms_all": [round(v, 3) for v in ms[1:]], "rows": a.rows,
                              "decode_steps": len(dec),
                              "decode_step_ms_median": round(statistics.median(dec), 4) if dec else None}), flush=True)
            del eng, meta
            gc.collect()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
