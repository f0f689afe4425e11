"""Prefill rope_and_cache at the bench's chunk shape (Llama-3-8B heads, 12 x 1365 tokens): time
with the paged K/V cache write, without it (rope only), and the cache write alone.

    python tools/bench_rope_cache.py [--seqs 12] [--len 1365]

``--qk-norm``: the plain form against the QK-norm form (Qwen3) at the Qwen3-8B / Llama-3-8B head
shape, alternating in one process, ``--reps`` timed windows each (median and range printed): 64
decode rows from 4 split-K slabs (400 calls captured in a hipGraph, so that the window is
device-bound), a 16384-token prefill chunk, and both over the fp8 cache.
``--plain-only`` times the plain form alone (the same windows; to compare two builds).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from k8s_llm_monitor_amd import ops  # noqa: E402
from k8s_llm_monitor_amd.ops import reference as ref  # noqa: E402

Hq, Hkv, D, BS = 32, 8, 128, 16


def _window(fn, iters: int) -> float:
    """Microseconds per call over one timed window (device events around ``iters`` calls)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _graphed(fn, iters: int):
    """``iters`` calls captured into one hipGraph: a replay is device-bound (a 4 us kernel launched
    eagerly measures the host's enqueue rate), as inside the engine's captured decode step."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g.replay


def _prefill_inputs(seqs: int, length: int, dev: str):
    T = seqs * length
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16)
    per = (length + BS - 1) // BS
    nb = seqs * per + 4
    pos = torch.arange(length, device=dev, dtype=torch.int32).repeat(seqs)
    blocks = torch.randperm(nb, device=dev)[: seqs * per].view(seqs, per).to(torch.int32)
    slots = (blocks[:, :, None] * BS + torch.arange(BS, device=dev, dtype=torch.int32)).view(seqs, -1)[:, :length]
    return qkv, pos, slots.reshape(-1).contiguous(), nb


def qk_norm_cases(a) -> None:
    dev = "cuda"
    cs = ref.rope_cos_sin(8192, D, 1e6, None, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    qk = None
    if not a.plain_only:
        qk = (torch.rand(D, device=dev, generator=g).to(torch.bfloat16) + 0.5,
              torch.rand(D, device=dev, generator=g).to(torch.bfloat16) + 0.5, 1e-6)
    ncol = (Hq + 2 * Hkv) * D
    # decode: 64 rows, each the last token of its own sequence, from 4 slabs
    B, S = 64, 4
    part = (torch.randn(S, B, ncol, device=dev, generator=g) * 0.3).reshape(-1)
    drow = torch.empty(B, ncol, device=dev, dtype=torch.bfloat16)
    dpos = torch.randint(100, 2000, (B,), device=dev, generator=g).to(torch.int32)
    dslots = (torch.randperm(B * 8, device=dev)[:B] * BS + dpos % BS).to(torch.int32)
    # prefill: 16 x 1024 tokens
    qkv, pos, slots, nb = _prefill_inputs(16, 1024, dev)
    nb = max(nb, B * 8)
    caches = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp8", torch.float8_e4m3fn)):
        al = ops.kv_cache_alloc(1, nb, Hkv, D, dt, dev)
        caches[name] = (al[0][0], al[1][0], al[2][0] if len(al) > 2 else None)

    def call(case: str, kv: str, norm: bool):
        kc, vc, sc = caches[kv]
        kw = {"qk_norm": qk} if norm else {}
        if case == "decode64_4slabs":
            return lambda: ops.rope_and_cache(drow, dpos, cs, kc, vc, dslots, Hq, Hkv, D, partial=part, nslabs=S,
                                              kv_scale=sc, **kw)
        return lambda: ops.rope_and_cache(qkv, pos, cs, kc, vc, slots, Hq, Hkv, D, kv_scale=sc, **kw)

    out = {"heads": [Hq, Hkv, D], "reps": a.reps}
    for case, iters in (("decode64_4slabs", 400), ("prefill16384", a.iters)):
        for kv in ("bf16", "fp8"):
            forms = [False] if a.plain_only else [False, True]
            fns = {f: call(case, kv, f) for f in forms}
            per, calls = 1, iters  # rope_and_cache calls per timed call, timed calls per window
            if case.startswith("decode"):
                per, calls = iters, 5
                fns = {f: _graphed(fn, per) for f, fn in fns.items()}
            for fn in fns.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            us = {f: [] for f in forms}
            for _ in range(a.reps):  # alternate the forms window by window
                for f in forms:
                    us[f].append(_window(fns[f], calls) / per)
            out[f"{case}_{kv}"] = {("qk_norm" if f else "plain"): {"median_us": round(statistics.median(v), 2),
                                                                  "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
                                   for f, v in us.items()}
    print(json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=12)
    ap.add_argument("--len", type=int, default=1365)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--qk-norm", action="store_true", help="plain against QK-norm form, decode / prefill / fp8 cache")
    ap.add_argument("--plain-only", action="store_true", help="with --qk-norm's cases: time the plain form alone")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.qk_norm or a.plain_only:
        return qk_norm_cases(a)
    T = a.seqs * a.len
    dev = "cuda"
    qkv, pos, slots, nb = _prefill_inputs(a.seqs, a.len, dev)
    kc = torch.zeros(nb, Hkv, D // 8, BS, 8, device=dev, dtype=torch.bfloat16)
    vc = torch.zeros(nb, Hkv, D, BS, device=dev, dtype=torch.bfloat16)
    cs = ref.rope_cos_sin(8192, D, 500000.0, None, device=dev)
    nbytes = {"cache": T * ((Hq + 2 * Hkv) * D * 2 + (Hq + Hkv) * D * 2 + 2 * Hkv * D * 2),
              "rope_only": T * (Hq + Hkv) * D * 2 * 2, "cache_only": T * 2 * Hkv * D * 2 * 2}
    cases = {"cache": (slots, True), "rope_only": (None, True), "cache_only": (slots, False)}
    out = {"T": T}
    for name, (sl, rope) in cases.items():
        for _ in range(3):
            ops.rope_and_cache(qkv, pos, cs, kc, vc, sl, Hq, Hkv, D, apply_rope=rope)
        torch.cuda.synchronize()
        us = _window(lambda: ops.rope_and_cache(qkv, pos, cs, kc, vc, sl, Hq, Hkv, D, apply_rope=rope), a.iters)
        out[name] = {"us": round(us, 1), "TBps": round(nbytes[name] / us / 1e6, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
