#!/usr/bin/env python
"""What an embedding request costs and what it saves (profiles/r27/README.md).

    python tools/bench_embed.py --mode kernel
    python tools/bench_embed.py --mode step [--model llama-3-8b --inputs 64 --lens 128,1600 --repeats 5]

``kernel``: ``ops.pool_l2`` alone at 64 x 4096 (bf16 rows, full width), 20 calls per captured graph,
the median of 5 timings of 20 replays.
``step``: one random-init engine (graphs, pipelined prefill, prefix caching off so that every wave
computes every token), waves of ``--inputs`` prompts of ``len`` random tokens.  After one unreported
warm-up wave of each kind, ``--repeats`` pairs of waves, alternating: ``embed`` (embedding requests -
no LM head, no sampler, no token) and ``gen1`` (the same prompts as generation requests with
``max_tokens=1`` - the same prefill, then the head over the last rows and the sampler).  A wave's GPU
time is taken between two events around it (the GPU is busy from the first launch to the last
read-back; the host's scheduling of the next step overlaps the running one); reported per kind: the
median wave time, the prefill steps of a wave, the time per step and inputs/s."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def kernel_mode(a) -> None:
    from k8s_llm_monitor_amd import ops

    dev = "cuda"
    R, d = 64, 4096
    x = torch.randn(R, d, device=dev).to(torch.bfloat16)
    dim = torch.full((R,), d, dtype=torch.int32, device=dev)
    out = torch.zeros(R, d, device=dev)
    ops.pool_l2(x, dim, out=out)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(20):
            ops.pool_l2(x, dim, out=out)
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / 400)
    print(json.dumps({"kernel": "pool_l2", "rows": R, "d": d, "us": round(statistics.median(ts), 2),
                      "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}), flush=True)


def step_mode(a) -> None:
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams

    eng = LLMEngine(EngineConfig(model=a.model, max_num_seqs=a.inputs, max_model_len=4096, kv_cache_gb=48.0, seed=1,
                                 prefix_caching=False), device="cuda")
    eng.warmup()
    g = torch.Generator().manual_seed(5)
    one = SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True)

    def wave(prompts, embed: bool):
        p0 = eng.counters["prefill_steps"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        seqs = [eng.add_request(p, None if embed else one, embed=True if embed else None) for p in prompts]
        while eng.has_work():
            eng.step()
        e1.record()
        torch.cuda.synchronize()
        want = "embed" if embed else "length"
        assert all(s.finish_reason == want for s in seqs), [s.finish_reason for s in seqs][:4]
        return e0.elapsed_time(e1), eng.counters["prefill_steps"] - p0

    for n in [int(x) for x in a.lens.split(",")]:
        prompts = [torch.randint(100, 120000, (n,), generator=g).tolist() for _ in range(a.inputs)]
        wave(prompts, True)
        wave(prompts, False)
        ms = {True: [], False: []}
        steps = {}
        for _ in range(a.repeats):
            for embed in (True, False):
                t, steps[embed] = wave(prompts, embed)
                ms[embed].append(t)
        for embed, label in ((True, "embed"), (False, "gen1")):
            med = statistics.median(ms[embed])
            print(json.dumps({"kind": label, "inputs": a.inputs, "len": n, "prefill_steps": steps[embed],
                              "wave_ms": round(med, 3), "min_ms": round(min(ms[embed]), 3),
                              "max_ms": round(max(ms[embed]), 3), "ms_per_step": round(med / steps[embed], 3),
                              "inputs_per_s": round(a.inputs * 1e3 / med, 1)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="step", choices=["step", "kernel"])
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--inputs", type=int, default=64)
    ap.add_argument("--lens", default="128,1600")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    (step_mode if a.mode == "step" else kernel_mode)(a)


if __name__ == "__main__":
    main()
