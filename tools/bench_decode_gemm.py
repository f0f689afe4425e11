"""Decode projections of a Llama-3-8B layer (+ the LM head) at decode batch M: the shipped
row-major skinny kernel (gemm_skinny_rm_kernel; hipBLASLt F.linear for the LM head) against the
shared-A decode GEMM (gemm_decode.hip) over its packed weight copies, for a list of launch
configurations (splits, n-tiles per wave, waves, ring depth).  One process, interleaved rounds;
each case is 32 hipGraph-captured calls rotating over > 512 MiB of weight copies, so weights
stream from HBM as in a decode step.  Every dec configuration is checked against an fp32
reference of the same product first (max |err| / max |ref|).  Above 64 rows (``--ms 64,96,128``:
the 5..8 m-tile instantiations) only gemm_decode.hip has a kernel: the row-major skinny case is
left out, hipBLASLt stays for the LM head, and configurations without a 65..128-row instantiation
(ops.dec_form_ok) are reported as errors and skipped.  ``pick`` lines give ops.dec_config's choice per row count.
``--wdtype fp8`` adds, next to every dec configuration with an fp8 form (ops.DEC_F8_FORMS), the
same launch over the fp8 encoding of the weights (``f8_`` cases: half the weight bytes; TBps
counts the bytes actually streamed), checked for bit equality with the bf16 launch over the
dequantised weights, which the bf16 cases then stream too.  ``--wdtype mxfp4`` does the same for
the MXFP4 encoding (``f4_`` cases, ops.DEC_F4_FORMS: 17/64 of the bytes), ``--wdtype fp8,mxfp4``
both in one session (each checked against the bf16 launch over its own dequantised weights;
the timed bf16 cases stream the last encoding's).  ``--f4-depths 8,16`` times the mxfp4 cases
once per forced F4 ring depth (ops.DEC_F4_DEPTH_FORCE; 0 = the launcher's choice) where the
launcher takes it.  ``--ops 70b_gate_up``, ``--ops q3_gate_up,q3_down,q3_lm_head`` (Qwen3-8B) etc.: SHAPES.
``--slab-sw 000,100,110,001,111``: every bf16 slab configuration once per setting of
(ops.DEC_SLAB_ROWS, DEC_SLAB_WT, DEC_XCD_SPLITS) - ``_sw`` cases, interleaved in one session.
``--experts E``: the grouped (grid.z = expert) launches of a Mixtral-8x7B MoE layer over E local
experts instead - gate_up and down (``--ops``), bf16 stacks on ops.dec_config's pick against the
``--wdtype`` code stacks on ops.dec_grouped_q_config's (and the bf16 stacks on that pick where it
differs), each quantised launch checked for bit equality with the bf16 launch of its configuration.

    python tools/bench_decode_gemm.py [--ms 1,32,64] [--ops qkv,o,gate_up,down,lm_head] [--rounds 3] [--wdtype fp8]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from k8s_llm_monitor_amd import ops  # noqa: E402
from tools.bench_skinny import timeit  # noqa: E402

D, FF, V = 4096, 14336, 128256
SHAPES = {"qkv": (6144, D, 0), "o": (D, D, 0), "gate_up": (2 * FF, D, 2), "down": (D, FF, 0), "lm_head": (V, D, 1),
          "70b_gate_up": (2 * 28672, 8192, 2),  # Llama-3-70B at TP=1
          # Qwen3-8B (qkv and o are Llama-3-8B's shapes)
          "q3_gate_up": (2 * 12288, D, 2), "q3_down": (D, 12288, 0), "q3_lm_head": (151936, D, 1)}
CFGS = {  # the sweep list: forms of ops.DEC_FORMS (another form: add its row to the table first)
    "qkv": [(4, 1, 6, 8), (8, 1, 8, 8), (4, 1, 4, 16), (4, 1, 4, 8)],
    "o": [(4, 1, 4, 16), (4, 1, 4, 8), (8, 1, 8, 8), (16, 1, 8, 8)],
    "gate_up": [(1, 1, 7, 16), (1, 1, 7, 8), (1, 1, 8, 16)],
    "down": [(4, 1, 4, 16), (4, 1, 4, 8), (8, 1, 8, 8), (4, 1, 8, 8)],
    "lm_head": [(1, 4, 8, 4), (1, 3, 8, 8), (1, 2, 8, 8)],
    "70b_gate_up": [(1, 1, 8, 16)],
    "q3_gate_up": [(1, 1, 7, 8), (1, 1, 7, 16), (1, 1, 8, 16)],
    "q3_down": [(8, 1, 8, 8), (4, 1, 4, 16), (4, 1, 8, 8)],
    "q3_lm_head": [(1, 4, 8, 4), (1, 3, 8, 8), (1, 2, 8, 8)],
}


def grouped(a, encs: list) -> None:
    """--experts: one MoE layer's grouped launches, bf16 against the quantised stacks."""
    dev, E = "cuda", a.experts
    for name in [n for n in a.ops.split(",") if n in ("gate_up", "down")]:
        N, K, epi = SHAPES[name]
        ncopy = max(2, (512 << 20) // (E * N * K * 2) + 1)
        enc_kw = {"fp8": dict(f8=True), "mxfp4": dict(f4=True)}
        picks = {"bf16": ops.dec_config(N, K, epi, experts=E)}
        picks.update({enc: ops.dec_grouped_q_config(N, K, epi, E, **enc_kw[enc]) for enc in encs})
        print(json.dumps({"op": name, "experts": E, "picks": picks}), flush=True)
        # encoding -> (code stacks per copy, scale stacks per copy, packed bf16 stack of copy 0's dequantised values);
        # the timed bf16 stacks hold the last encoding's dequantised values (one model, two encodings)
        stacks: dict = {enc: ([], [], None) for enc in encs}
        wdec = []
        for i in range(ncopy):
            ws = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(E)]
            for enc in encs:
                if enc == "fp8":
                    qs = [ops.quantize_rows_fp8(w) for w in ws]
                    dq = [ops.dequantize_rows_fp8(q, sc) for q, sc in qs]
                    pk = [(ops.pack_skinny_f8(q), sc) for q, sc in qs]
                else:
                    qs = [ops.quantize_mxfp4(w) for w in ws]
                    dq = [ops.dequantize_mxfp4(q, sc) for q, sc in qs]
                    pk = [ops.pack_skinny_f4(q, sc) for q, sc in qs]
                stacks[enc][0].append(torch.stack([q for q, _ in pk]))
                stacks[enc][1].append(torch.stack([sc for _, sc in pk]))
                if i == 0:
                    stacks[enc] = stacks[enc][:2] + (torch.stack([ops.pack_skinny(w) for w in dq]),)
                if enc == encs[-1]:
                    ws = dq
                del qs, dq, pk
            wdec.append(torch.stack([ops.pack_skinny(w) for w in ws]))
            del ws
        gb = E * N * K * 2 / 1e9
        for M in map(int, a.ms.split(",")):
            MT = -(-M // 16)
            if epi == 2:
                xa = ops.pack_activation(torch.randn(M, K, device=dev, dtype=torch.bfloat16))
                out = dict(out=torch.empty((E, MT, N // 64, 64, 8), device=dev, dtype=torch.bfloat16))
            else:
                xa = torch.stack([ops.pack_activation(torch.randn(M, K, device=dev, dtype=torch.bfloat16)) for _ in range(E)])
                rw = torch.rand(M, E, device=dev)
                out = dict(workspace=torch.empty(E * M * N, device=dev, dtype=torch.float32), row_w=rw)
            res_t = out["out"] if epi == 2 else out["workspace"]
            cases = {}
            for cfg in dict.fromkeys(c for c in picks.values() if c is not None):
                cases["bf16_" + "_".join(map(str, cfg))] = (
                    lambda i, cfg=cfg: ops.dec_gemm_grouped(xa, wdec[i % ncopy], epi, M, cfg=cfg, **out))
            for enc in encs:
                cfg = picks[enc]
                if cfg is None:
                    continue
                ops.dec_gemm_grouped(xa, stacks[enc][2], epi, M, cfg=cfg, **out)
                want = res_t.clone()
                ops.dec_gemm_grouped_q(xa, stacks[enc][0][0], stacks[enc][1][0], epi, M, cfg=cfg, **out)
                print(json.dumps({"op": name, "experts": E, "M": M, "cfg": cfg,
                                  enc + "_bit_equal_to_bf16": torch.equal(want, res_t)}), flush=True)
                cases[enc + "_" + "_".join(map(str, cfg))] = (
                    lambda i, cfg=cfg, enc=enc: ops.dec_gemm_grouped_q(xa, stacks[enc][0][i % ncopy],
                                                                       stacks[enc][1][i % ncopy], epi, M, cfg=cfg, **out))
            res: dict = {}
            for _ in range(a.rounds):
                for tag, fn in cases.items():
                    res.setdefault(tag, []).append(timeit(fn, a.iters))
            for tag, ts in res.items():
                t = min(ts)
                b = gb / 2 if tag.startswith("fp8_") else gb * 17 / 64 if tag.startswith("mxfp4_") else gb
                print(json.dumps({"op": name, "experts": E, "M": M, "impl": tag, "us": round(t, 2),
                                  "us_all": [round(v, 2) for v in ts], "TBps": round(b / t * 1e3, 2)}), flush=True)
        del wdec, stacks
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=320)
    ap.add_argument("--ms", default="1,32,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ops", default="qkv,o,gate_up,down,lm_head")
    ap.add_argument("--cfgs", default=None, help="op:S,NTW,W,D|S,NTW,W,D;... overrides the sweep list")
    ap.add_argument("--wdtype", default="bf16", help="bf16, fp8, mxfp4 or fp8,mxfp4")
    ap.add_argument("--f4-depths", default="0", help="F4 ring depths to time the mxfp4 cases at (0 = automatic)")
    ap.add_argument("--no-base", action="store_true", help="leave out the row-major skinny / hipBLASLt case")
    ap.add_argument("--experts", type=int, default=0, help="E > 0: the grouped launches of a Mixtral MoE layer")
    ap.add_argument("--slab-sw", default=None,
                    help="time every bf16 slab configuration once per setting of (ops.DEC_SLAB_ROWS, DEC_SLAB_WT, "
                         "DEC_XCD_SPLITS), e.g. 000,100,110,001,111 (digits 0 / 1; s = as shipped)")
    a = ap.parse_args()
    encs = [e for e in a.wdtype.split(",") if e != "bf16"]
    if any(e not in ("fp8", "mxfp4") for e in encs):
        ap.error("--wdtype: bf16, fp8, mxfp4 or fp8,mxfp4")
    f4_depths = [int(d) for d in a.f4_depths.split(",")]
    dev = "cuda"
    torch.manual_seed(0)
    if a.experts:
        return grouped(a, encs)
    cfgs = dict(CFGS)
    if a.cfgs:
        for item in a.cfgs.split(";"):
            op, c = item.split(":")
            cfgs[op] = [tuple(int(v) for v in cc.split(",")) for cc in c.split("|")]
    for name in a.ops.split(","):
        N, K, epi = SHAPES[name]
        ncopy = max(2, (512 << 20) // (N * K * 2) + 1)
        wrm = [(torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02) for _ in range(ncopy)]
        if epi == 2:  # the engine's resident w13 is [64 gate | 64 up]-interleaved; the dec copy by 8
            canon = [ops.deinterleave_gate_up(w) for w in wrm]
            wdec = [ops.pack_skinny(ops.interleave_gate_up8(w)) for w in canon]
        else:
            wdec = [ops.pack_skinny(w) for w in wrm]
        wq = ws = None
        quant: dict = {}  # encoding -> (codes per copy, scales per copy, packed bf16 dequantised values of copy 0)
        for enc in encs:  # one model, two encodings: the bf16 copies become the dequantised values
            if enc == "fp8":
                qs = [ops.quantize_rows_fp8(ops.unpack_skinny(w)) for w in wdec]
                dq = [ops.pack_skinny(ops.dequantize_rows_fp8(q, s)) for q, s in qs]
                quant[enc] = ([ops.pack_skinny_f8(q) for q, _ in qs], [s for _, s in qs], dq[0])
            else:
                qs = [ops.quantize_mxfp4(ops.unpack_skinny(w)) for w in wdec]
                dq = [ops.pack_skinny(ops.dequantize_mxfp4(q, s)) for q, s in qs]
                pk = [ops.pack_skinny_f4(q, s) for q, s in qs]
                quant[enc] = ([c for c, _ in pk], [s for _, s in pk], dq[0])
                del pk
            del qs
            if enc == encs[-1]:
                wdec = dq
                wrm = [ops.interleave_gate_up(ops.deinterleave_gate_up8(ops.unpack_skinny(w))) if epi == 2
                       else ops.unpack_skinny(w) for w in wdec]
            del dq
        gb = N * K * 2 / 1e9
        for M in map(int, a.ms.split(",")):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            xp = ops.pack_activation(x)
            ref = x.float() @ wrm[0].float().t()
            if epi == 2:
                g, u = ops._cpu_deinterleave(ref.to(torch.bfloat16).float())
                ref = F.silu(g) * u
            scale = ref.abs().max().item()
            wsp = torch.empty(16 * M * N, device=dev, dtype=torch.float32)
            act = ops.packed_empty(M, N // 2, torch.bfloat16, dev)
            yb = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def dec_out(cfg, w=None, **kw):
                w = wdec[0] if w is None else w
                if epi == 0:
                    s = ops.dec_gemm(xp, w, 0, M, workspace=wsp, cfg=cfg, **kw)
                    return wsp[: s * M * N].view(s, M, N).sum(0)
                if epi == 1:
                    ops.dec_gemm(xp, w, 1, M, out=yb, cfg=cfg, **kw)
                    return yb.float()
                ops.dec_gemm(xp, w, 2, M, out=act, cfg=cfg, **kw)
                return ops.unpack_skinny(act)[:M].float()

            cases = {}
            print(json.dumps({"op": name, "M": M, "pick": ops.dec_config(N, K, epi, rows=M)}), flush=True)
            if a.no_base or (M > ops.SKINNY_MAX_M and epi != 1):
                pass  # gemm_skinny stops at 64 rows
            elif epi == 0:
                cases["rm"] = lambda i: ops.skinny_slabs(xp, wrm[i % ncopy], wsp, 0, rows=M)
            elif epi == 2:
                cases["rm"] = lambda i: ops.skinny_swiglu(xp, wrm[i % ncopy], out=act, rows=M, packed_out=True)
            else:
                cases["hipblaslt"] = lambda i: torch.matmul(x, wrm[i % ncopy].t(), out=yb)
            for cfg in cfgs[name]:
                if not ops.dec_form_ok(epi, cfg, M):
                    print(json.dumps({"op": name, "M": M, "cfg": cfg,
                                      "error": f"gemm_dec: form {(epi,) + cfg[1:]} not compiled for {M} rows"}),
                          flush=True)
                    continue
                err = (dec_out(cfg) - ref).abs().max().item() / max(scale, 1e-6)
                tag = "dec" + "_".join(map(str, cfg))

                def run_sw(i, cfg=cfg, sw=None):
                    if sw is not None:
                        ops.DEC_SLAB_ROWS, ops.DEC_SLAB_WT, ops.DEC_XCD_SPLITS = sw
                    try:
                        return ops.dec_gemm(xp, wdec[i % ncopy], epi, M, workspace=wsp, out=act if epi == 2 else yb, cfg=cfg)
                    finally:
                        ops.DEC_SLAB_ROWS = ops.DEC_SLAB_WT = ops.DEC_XCD_SPLITS = -1

                if a.slab_sw and epi == 0:
                    for word in a.slab_sw.split(","):
                        sw = tuple(-1 if ch == "s" else int(ch) for ch in word)
                        cases[tag + "_sw" + word] = (lambda i, run_sw=run_sw, sw=sw: run_sw(i, sw=sw))
                else:
                    cases[tag] = run_sw
                print(json.dumps({"op": name, "M": M, "cfg": cfg, "rel_err": round(err, 5)}), flush=True)
                for enc, (wq, ws, wchk) in quant.items():
                    pre, kw = ("f8_", dict(f8=True)) if enc == "fp8" else ("f4_", dict(f4=True, K=K))
                    if not ops.dec_form_ok(epi, cfg, M, **kw):
                        continue
                    same = torch.equal(dec_out(cfg, wchk).clone(), dec_out(cfg, wq[0], wscale=ws[0]))
                    print(json.dumps({"op": name, "M": M, "cfg": cfg, pre + "bit_equal_to_bf16": same}), flush=True)

                    def run(i, cfg=cfg, wq=wq, ws=ws, depth=0):
                        ops.DEC_F4_DEPTH_FORCE = depth
                        try:
                            return ops.dec_gemm(xp, wq[i % ncopy], epi, M, workspace=wsp, out=act if epi == 2 else yb,
                                                cfg=cfg, wscale=ws[i % ncopy])
                        finally:
                            ops.DEC_F4_DEPTH_FORCE = 0

                    for d in (f4_depths if enc == "mxfp4" else [0]):
                        fn = (lambda i, run=run, d=d: run(i, depth=d))
                        try:
                            fn(0)  # a forced depth the launcher does not take for this slice: left out
                        except RuntimeError:
                            continue
                        cases[pre + (f"ring{d}_" if d else "") + tag] = fn
            res: dict = {}
            for _ in range(a.rounds):
                for tag, fn in cases.items():
                    res.setdefault(tag, []).append(timeit(fn, a.iters))
            for tag, ts in res.items():
                t = min(ts)
                b = gb / 2 if tag.startswith("f8_") else gb * 17 / 64 if tag.startswith("f4_") else gb
                print(json.dumps({"op": name, "M": M, "impl": tag, "us": round(t, 2),
                                  "us_all": [round(v, 2) for v in ts], "TBps": round(b / t * 1e3, 2)}), flush=True)
        del wrm, wdec, wq, ws, quant
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
