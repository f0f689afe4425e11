#!/usr/bin/env python
"""What e4m3 weights cost in accuracy: the logits of a model whose dense projections and LM head
were quantised per row (decode_weights="fp8": its bf16 weights are the dequantised values) against
the same seeded model unquantised, teacher-forced over a few prompts.  Prints one JSON line: max and
rms logit difference, the logit scale, and how many of the rows keep their argmax.

    python tools/fp8_logit_diff.py [--model llama-3-8b --layers 2 --prompts 8]

``--decode-weights mxfp4`` (or ``fp8,mxfp4``: one line each against the same unquantised engine)
measures the MXFP4 encoding (ops.quantize_mxfp4: round-to-nearest e2m1, one e8m0 scale per 32
weights) the same way.  ``--model mixtral-8x7b --layers 2``: a MoE model, whose expert stacks
(97 % of its weights) are quantised expert by expert under the same two recipes.

(``prefill_weights: fp8`` needs no numbers of its own: it releases the bf16 copy of weights whose
values stay exactly these dequantised ones, and its prefill GEMM is bit-identical.)

``--kv-cache-dtype fp8`` measures the e4m3 KV cache instead: both engines keep bf16 weights, one
on a bf16 and one on an fp8 cache; the first half of each prompt is prefilled into the engine's own
paged cache and the second half decoded through it one teacher-forced token at a time, so every
logit row compared has read quantised keys and values.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--kv-cache-dtype", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--decode-weights", default="fp8", help="the weight encodings to measure: fp8, mxfp4 or fp8,mxfp4")
    a = ap.parse_args()
    kv_mode = a.kv_cache_dtype == "fp8"
    encs = a.decode_weights.split(",")
    if any(e not in ("fp8", "mxfp4") for e in encs) or (kv_mode and encs != ["fp8"]):
        ap.error("--decode-weights: fp8, mxfp4 or fp8,mxfp4 (without --kv-cache-dtype fp8)")
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine
    from k8s_llm_monitor_amd.models import AttnMeta

    def engine(dw):
        return LLMEngine(EngineConfig(model=a.model, model_overrides={"n_layers": a.layers} if a.layers else {},
                                      max_num_seqs=8, max_model_len=1024, kv_cache_gb=1.0, seed=a.seed,
                                      decode_weights="bf16" if kv_mode else dw,
                                      kv_cache_dtype=dw if kv_mode else "bf16", use_graphs=False), device="cuda")

    def through_cache(e, ids):
        """Logits of rows h - 1 .. len - 1: ids[:h] prefilled into e's cache, the rest decoded through it."""
        k, h = len(ids), max(1, len(ids) // 2)
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")  # noqa: E731
        bt = torch.arange(1, (k + 15) // 16 + 1, dtype=torch.int32, device="cuda")[None]
        pos = torch.arange(k, dtype=torch.int32, device="cuda")
        slots = (bt[0][(pos // 16).long()] * 16 + pos % 16).to(torch.int32)
        meta = AttnMeta(is_prefill=True, positions=pos[:h], slot_mapping=slots[:h], cu_seqlens=i32([0, h]),
                        logits_idx=torch.tensor([h - 1], device="cuda"))
        out = [e.model.forward(i32(ids[:h]), meta, e.runner.kv).float()]
        for t in range(h, k):
            meta = AttnMeta(is_prefill=False, positions=pos[t:t + 1], slot_mapping=slots[t:t + 1], block_tables=bt,
                            seq_lens=i32([t + 1]), decode_ws=e.runner.decode_ws)
            out.append(e.model.forward(i32(ids[t:t + 1]), meta, e.runner.kv).float())
        return torch.cat(out)

    def logits(e, ids):
        t = torch.tensor(ids, dtype=torch.int32, device="cuda")
        k = len(ids)
        meta = AttnMeta(is_prefill=True, positions=torch.arange(k, dtype=torch.int32, device="cuda"),
                        slot_mapping=torch.full((k,), -1, dtype=torch.int32, device="cuda"),
                        cu_seqlens=torch.tensor([0, k], dtype=torch.int32, device="cuda"),
                        logits_idx=torch.arange(k, device="cuda"))
        with torch.no_grad():
            return through_cache(e, ids) if kv_mode else e.model.forward(t, meta, None).float()

    base = engine("bf16")
    prompts = [f"a node-{i:03d} CPU={30 + i % 60}% pod payments-{i} restarts={i % 7} 为什么我的pod频繁重启？"
               for i in range(a.prompts)]
    ids_all = [base.tokenizer.encode(p) for p in prompts]
    ref = [logits(base, ids) for ids in ids_all]
    for enc in encs:
        e = engine(enc)
        d2 = n = same = rows = 0
        dmax = scale = 0.0
        for ids, lb in zip(ids_all, ref):
            lq = logits(e, ids)
            diff = lq - lb
            d2 += float(diff.pow(2).sum())
            n += diff.numel()
            dmax = max(dmax, float(diff.abs().max()))
            scale = max(scale, float(lb.abs().max()))
            same += int((lq.argmax(-1) == lb.argmax(-1)).sum())
            rows += diff.shape[0]
        print(json.dumps({"model": a.model, "layers": a.layers, "quantised": "kv_cache" if kv_mode else "weights",
                          "encoding": enc, "prompts": a.prompts, "rows": rows,
                          "logit_scale": round(scale, 4), "max_diff": round(dmax, 4),
                          "rms_diff": round((d2 / n) ** 0.5, 5), "argmax_kept": same}), flush=True)
        del e
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
