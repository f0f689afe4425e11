#!/usr/bin/env python
"""What e4m3 weights cost in accuracy: the logits of a model whose dense projections and LM head
were quantised per row (decode_weights="fp8": its bf16 weights are the dequantised values) against
the same seeded model unquantised, teacher-forced over a few prompts.  Prints one JSON line: max and
rms logit difference, the logit scale, and how many of the rows keep their argmax.

    python tools/fp8_logit_diff.py [--model llama-3-8b --layers 2 --prompts 8]
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
    a = ap.parse_args()
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine
    from k8s_llm_monitor_amd.models import AttnMeta

    def engine(dw):
        return LLMEngine(EngineConfig(model=a.model, model_overrides={"n_layers": a.layers} if a.layers else {},
                                      max_num_seqs=8, max_model_len=1024, kv_cache_gb=1.0, seed=a.seed,
                                      decode_weights=dw, use_graphs=False), device="cuda")

    engs = {dw: engine(dw) for dw in ("bf16", "fp8")}
    prompts = [f"a node-{i:03d} CPU={30 + i % 60}% pod payments-{i} restarts={i % 7} 为什么我的pod频繁重启？"
               for i in range(a.prompts)]
    d2 = n = same = rows = 0
    dmax = scale = 0.0
    for p in prompts:
        ids = engs["bf16"].tokenizer.encode(p)
        lg = {}
        for dw, e in engs.items():
            t = torch.tensor(ids, dtype=torch.int32, device="cuda")
            k = len(ids)
            meta = AttnMeta(is_prefill=True, positions=torch.arange(k, dtype=torch.int32, device="cuda"),
                            slot_mapping=torch.full((k,), -1, dtype=torch.int32, device="cuda"),
                            cu_seqlens=torch.tensor([0, k], dtype=torch.int32, device="cuda"),
                            logits_idx=torch.arange(k, device="cuda"))
            with torch.no_grad():
                lg[dw] = e.model.forward(t, meta, None).float()
        diff = lg["fp8"] - lg["bf16"]
        d2 += float(diff.pow(2).sum())
        n += diff.numel()
        dmax = max(dmax, float(diff.abs().max()))
        scale = max(scale, float(lg["bf16"].abs().max()))
        same += int((lg["fp8"].argmax(-1) == lg["bf16"].argmax(-1)).sum())
        rows += diff.shape[0]
    print(json.dumps({"model": a.model, "layers": a.layers, "prompts": a.prompts, "rows": rows,
                      "logit_scale": round(scale, 4), "max_diff": round(dmax, 4),
                      "rms_diff": round((d2 / n) ** 0.5, 5), "argmax_kept": same}), flush=True)


if __name__ == "__main__":
    main()
