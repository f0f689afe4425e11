"""Fused operators.  GPU tensors run the gfx950 HIP kernels of ``_k8sllm_ops`` (built in-tree by
``python -m k8s_llm_monitor_amd.ops.build``); CPU tensors run the fp32 references of
:mod:`.reference` (attention: the batched SDPA forms of :mod:`.cpu_attn`, same math).  A GPU tensor never silently falls back: if the extension is missing on a
GPU box the call raises, so tests and benchmarks always exercise the native kernels.
"""
from __future__ import annotations

import importlib
import math
from collections import OrderedDict
from typing import Optional

import torch

from . import cpu_attn
from . import reference as ref

_EXT = None
_EXT_ERR: Optional[BaseException] = None


def native():
    """The compiled extension module (raises with the build hint if unavailable)."""
    global _EXT, _EXT_ERR
    if _EXT is None and _EXT_ERR is None:
        try:
            _EXT = importlib.import_module("k8s_llm_monitor_amd.ops._k8sllm_ops")
        except BaseException as e:  # noqa: BLE001 - remember why, re-raise on GPU use
            _EXT_ERR = e
    if _EXT is None:
        raise RuntimeError(
            "gfx950 kernels (_k8sllm_ops) are not built/loadable; run "
            "`python -m k8s_llm_monitor_amd.ops.build` (cause: %r)" % (_EXT_ERR,))
    return _EXT


def native_available() -> bool:
    try:
        native()
        return True
    except RuntimeError:
        return False


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


# ---------------------------------------------------------------- norms / activations

def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if not _gpu(x):
        r = ref.rms_norm(x, w, eps)
        return out.copy_(r) if out is not None else r
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    native().rms_norm(out, x, w, eps)
    return out


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """residual <- x + residual (bf16); returns rms_norm(residual) * w."""
    if not _gpu(x):
        y, s = ref.fused_add_rms_norm(x, residual, w, eps)
        residual.copy_(s)
        return out.copy_(y) if out is not None else y
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    if x.numel():  # no rows (a prefill step without logit rows): nothing to launch
        native().fused_add_rms_norm(out, x, residual, w, eps)
    return out


# ---------------------------------------------------------------- decode projections (skinny GEMM)

# The compiled forms of the shared-A decode GEMM: (epilogue, n-tiles per wave, waves, ring depth,
# max m-tiles, wide-norm) - the rows of kDecForms in csrc/gemm_dec_forms.h, which
# native().gemm_dec_forms() reports (tests/test_decode_rows_cpu.py compares the two).  A form
# serves up to 16 * max m-tiles rows; wide-norm: also the deferred-norm form over per-16-column
# sums (behind dec_gemm_rc).  Kept here as well because dec_config runs without the extension.
# The order is dec_config's candidate order: the first of two equal candidates wins.
DEC_SLAB, DEC_BF16, DEC_SWIGLU8 = 0, 1, 2
DEC_FORMS: tuple = (
    (DEC_SLAB, 1, 8, 8, 8, 0),
    (DEC_SLAB, 1, 6, 8, 8, 0),
    (DEC_SLAB, 1, 4, 16, 4, 0),
    (DEC_SLAB, 1, 4, 8, 8, 0),
    (DEC_SWIGLU8, 1, 7, 8, 8, 1),
    (DEC_SWIGLU8, 1, 7, 16, 4, 1),
    (DEC_SWIGLU8, 1, 8, 16, 4, 0),
    (DEC_BF16, 4, 8, 4, 4, 0),
    (DEC_BF16, 3, 8, 8, 4, 0),
    (DEC_BF16, 2, 8, 8, 8, 0),
    (DEC_BF16, 1, 8, 8, 4, 0),
)
# compiled, but never an automatic pick: only DEC_TABLE / DEC_TABLE_M128 (qkv) name it
DEC_FORMS_TABLE_ONLY = frozenset({(DEC_SLAB, 1, 6, 8)})

# Row limits of the decode GEMMs, all in one place:
#   64  gemm_skinny, the grouped (MoE) shared-A launches (dec_gemm_grouped), the wide-norm form,
#       the row-complete o projection (dec_gemm_rc, used up to 32 rows) and every TP > 1 decode
#       tail;
#   128 the dense shared-A decode GEMM (dec_gemm: the forms of 8 m-tiles) - dense Llama-family
#       models at TP=1 over the packed weights (CausalLM.dec_rows_max).
# mirrors of kSkinnyMaxM / kSkinnyGroupedMaxM (csrc/gemm_skinny_plan.h); tests/test_skinny_pack.py
# compares them with the extension's
SKINNY_MAX_M = 64
SKINNY_GROUPED_MAX_M = 128  # grouped (expert) launches over row-major weights
DEC_NARROW_MAX_M = 64  # kDecNarrowMaxM: grouped and wide-norm launches of gemm_dec_kernel
DEC_MAX_M = max(16 * f[4] for f in DEC_FORMS)  # dec_gemm (dense launches of gemm_dec_kernel)


def dec_row_classes() -> tuple:
    """The distinct row limits of the compiled forms, ascending: dec_config can answer differently
    from one class to the next and never within one."""
    return tuple(sorted({16 * f[4] for f in DEC_FORMS}))


def dec_form_ok(epi: int, cfg: tuple, rows: int, grouped: bool = False, wide_norm: bool = False,
                f8: bool = False, f4: bool = False, K: int = 0) -> bool:
    """Whether gemm_decode.hip has an instantiation for ``cfg = (splits, ntw, waves, depth)`` at
    ``rows`` rows: a DEC_FORMS row with that many m-tiles; ``grouped`` launches and the
    ``wide_norm`` form (which the row must have) stop at DEC_NARROW_MAX_M rows.  ``f8``: over fp8
    weights - a row listed in DEC_F8_FORMS, dense launches with the narrow deferred norm only.
    ``f4``: over mxfp4 weights - a row listed in DEC_F4_FORMS, the same limits; with ``K`` given,
    every split-K slice must also hold whole 256-deep A chunks (so whole 128-deep code groups)."""
    if (grouped or wide_norm) and (f8 or f4 or rows > DEC_NARROW_MAX_M):
        return False
    if f4:
        if dec_f4_depth(epi, cfg) == 0 or (K and (K % cfg[0] or (K // cfg[0]) % 256)):
            return False
    forms = [DEC_FORMS[i] for i in DEC_F8_FORMS] if f8 else [DEC_FORMS[i] for i, _ in DEC_F4_FORMS] if f4 else DEC_FORMS
    return any(f[:4] == (epi,) + tuple(cfg[1:]) and rows <= 16 * f[4] and (f[5] or not wide_norm) for f in forms)


# ---------------------------------------------------------------- fp8 (e4m3) decode weights
# One model, two encodings: a weight row is stored as OCP e4m3 codes times a power-of-two scale
# 2^e, e = ceil(log2(amax_row / 448)).  Every dequantised value code * 2^e is a bf16 value, so the
# bf16 tensors of an fp8-decoding model hold exactly what the fp8 kernel computes with, and the
# scale commutes with every rounding of the decode GEMM (applied to the fp32 accumulator).

# the DEC_FORMS rows (indices) that gemm_decode.hip also instantiates over fp8 weights: kDecF8Forms
# in csrc/gemm_dec_forms.h, reported by native().gemm_dec_f8_forms()
DEC_F8_FORMS: tuple = (0, 1, 4, 6, 7, 9)
FP8_MAX = 448.0  # largest finite e4m3fn magnitude


def quantize_rows_fp8(w: torch.Tensor) -> tuple:
    """Row-major weight [N, K] -> (codes [N, K] float8_e4m3fn, scale [N] fp32): per output row the
    power-of-two scale 2^e with e = ceil(log2(amax / 448)) (0 for an all-zero row) and
    code = w / 2^e rounded to e4m3 as ``Tensor.to(torch.float8_e4m3fn)`` rounds.  |w / 2^e| <= 448,
    so no code is NaN."""
    wf = w.float()
    m, x = torch.frexp(wf.abs().amax(dim=1) / FP8_MAX)  # amax / 448 = m 2^x, m in [0.5, 1) (0, 0 for zero)
    e = torch.where(m == 0.5, x - 1, x).clamp(-100, 119).to(torch.int32)
    scale = ((e + 127) << 23).view(torch.float32)  # 2^e exactly
    return (wf / scale[:, None]).to(torch.float8_e4m3fn), scale


def dequantize_rows_fp8(codes: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """code * 2^e per row, exact in bf16 (an e4m3 value has 4 significant bits)."""
    return (codes.float() * scale.float()[:, None]).to(dtype)


# ---- FP8 (e4m3) KV cache.  THE definition of the format; the kernels (csrc/common.h), the CPU
# references and the engine mirror it.  Codes sit in the bf16 cache's index order, one byte per
# element; kv_scale [.., NB, Hkv, 2, 16] fp32 holds one power-of-two scale per (token, kv head):
# [.., 0, t] for K (after RoPE), [.., 1, t] for V of block token t, tokens in sequence order.
KV_BLOCK = 16
KV_EXP_MAX = 60  # |e| <= 60: 2^e, 2^-e and every code * 2^e stay normal bf16 / fp32 numbers


def quantize_kv(x: torch.Tensor) -> tuple:
    """[T, Hkv, D] -> (codes [T, Hkv, D] float8_e4m3fn, scale [T, Hkv] fp32): the rule of
    :func:`quantize_rows_fp8` over the D values of one token and kv head, e = ceil(log2(amax / 448))
    clamped to [-60, 60] (0 for an all-zero vector), scale = 2^e, code = x / 2^e rounded to e4m3."""
    xf = x.float()
    m, ex = torch.frexp(xf.abs().amax(dim=-1) / FP8_MAX)
    e = torch.where(m == 0.5, ex - 1, ex).clamp(-KV_EXP_MAX, KV_EXP_MAX).to(torch.int32)
    scale = ((e + 127) << 23).view(torch.float32)
    return (xf / scale[..., None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn), scale


def dequantize_kv(codes: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """code * 2^e, exact in bf16."""
    return (codes.float() * scale.float()[..., None]).to(dtype)


def kv_cache_alloc(L: int, nb: int, hkv: int, D: int, dtype, device) -> tuple:
    """The paged KV cache of ``L`` layers and ``nb`` 16-token blocks, zeroed - the single owner of
    its layout: (k_cache [L, nb, Hkv, D/8, 16, 8], v_cache [L, nb, Hkv, D, 16] with a block's tokens
    in v_perm order), and for ``dtype=torch.float8_e4m3fn`` also kv_scale [L, nb, Hkv, 2, 16] fp32."""
    k = torch.zeros(L, nb, hkv, D // 8, KV_BLOCK, 8, dtype=dtype, device=device)
    v = torch.zeros(L, nb, hkv, D, KV_BLOCK, dtype=dtype, device=device)
    if dtype != torch.float8_e4m3fn:
        return k, v
    return k, v, torch.zeros(L, nb, hkv, 2, KV_BLOCK, dtype=torch.float32, device=device)


def kv_bytes_per_block(L: int, hkv: int, D: int, dtype) -> int:
    """Bytes one 16-token block takes over all layers: K + V elements, plus the scales for fp8."""
    n = 2 * L * hkv * D * KV_BLOCK * torch.empty(0, dtype=dtype).element_size()
    if dtype == torch.float8_e4m3fn:
        n += L * hkv * 2 * KV_BLOCK * 4
    return n


def pack_skinny_f8(q: torch.Tensor) -> torch.Tensor:
    """e4m3 codes [N, K] -> the fragment-packed [N/16, K/64, 64, 16] layout of gemm_dec's fp8 form:
    block (n-tile j, k-step pair p) holds, for lane l = 16 q + r, the 8 codes
    W[16 j + r, 64 p + 8 q : +8] (k-step 2p, pack_skinny's fragment order) followed by the 8 codes
    W[16 j + r, 64 p + 32 + 8 q : +8] (k-step 2p + 1): 1 KiB contiguous per block, two k-steps."""
    N, K = q.shape
    if N % 16 or K % 64:
        raise ValueError(f"pack_skinny_f8: [{N}, {K}] needs N % 16 == 0 and K % 64 == 0")
    b = q.contiguous().view(torch.uint8).reshape(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5)
    return b.reshape(N // 16, K // 64, 64, 16).contiguous().view(torch.float8_e4m3fn)


def unpack_skinny_f8(qp: torch.Tensor) -> torch.Tensor:
    nt, kp = qp.shape[0], qp.shape[1]
    b = qp.contiguous().view(torch.uint8).reshape(nt, kp, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5)
    return b.reshape(nt * 16, kp * 64).contiguous().view(torch.float8_e4m3fn)


def is_fp8(w: Optional[torch.Tensor]) -> bool:
    return w is not None and w.dtype == torch.float8_e4m3fn


# ---------------------------------------------------------------- MXFP4 decode weights
# The OCP microscaling format: e2m1 elements (sign in bit 3, grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}), one
# e8m0 power-of-two scale 2^(b - 127) per block of 32 along K, 4.25 bits per weight.  As with e4m3
# every dequantised value code * 2^e is a bf16 value, so the bf16 tensors of an mxfp4-decoding
# model hold exactly what the mxfp4 kernel computes with.

# the DEC_FORMS rows that gemm_decode.hip also instantiates over mxfp4 weights, as (index, F4 ring
# depth in k-steps at <= 16 rows - 8 above, and where it does not divide the K slice): kDecF4Forms
# in csrc/gemm_dec_forms.h, reported by native().gemm_dec_f4_forms()
DEC_F4_FORMS: tuple = ((0, 16), (1, 16), (4, 16), (7, 8), (9, 16))
# test / tool override: the F4 ring depth of every mxfp4 launch (0 = the launcher's choice)
DEC_F4_DEPTH_FORCE = 0
MXFP4_MAX = 6.0  # largest e2m1 magnitude
MXFP4_BLOCK = 32  # elements along K that share a scale
MXFP4_EXP_MAX = 60  # |e| <= 60: 2^e and every code * 2^e stay normal bf16 / fp32 numbers
_MXFP4_CHUNK = 1 << 25  # elements quantised / dequantised at a time
_E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def dec_f4_depth(epi: int, cfg: tuple) -> int:
    """The one-m-tile F4 ring depth (k-steps) of the DEC_F4_FORMS row of
    ``cfg = (splits, ntw, waves, depth)``, 0 where the form has no mxfp4 instantiation."""
    for i, d4 in DEC_F4_FORMS:
        if DEC_FORMS[i][:4] == (epi,) + tuple(cfg[1:]):
            return d4
    return 0


def quantize_mxfp4(w: torch.Tensor) -> tuple:
    """Row-major weight [N, K] -> (codes [N, K/2] uint8, scales [N, K/32] uint8).  Per (row, block of
    32 along K) the scale 2^e with e = ceil(log2(amax / 6)) clamped to +-60 (0 for a block of zeros),
    stored as the e8m0 byte e + 127; element = w / 2^e rounded to the nearest e2m1 value, ties to
    the even mantissa, sign in bit 3 (-0 stays -0).  |w / 2^e| <= 6, so nothing clips.  Element 2i
    sits in the low nibble of byte i."""
    N, K = w.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"quantize_mxfp4: [{N}, {K}] needs K % 32 == 0")
    rows = max(1, _MXFP4_CHUNK // K)
    if N > rows:  # an LM head: row chunks keep the fp32 / index temporaries small
        parts = [quantize_mxfp4(w[i:i + rows]) for i in range(0, N, rows)]
        return torch.cat([c for c, _ in parts]), torch.cat([s for _, s in parts])
    wf = w.float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    # amax = m 2^x, m in [0.5, 1): amax <= 6 * 2^e = 0.75 * 2^(e + 3) first holds at e = x - 3 for
    # m <= 0.75 and at x - 2 above (exact: no division); frexp(0) = (0, 0) gives the clamp's -3 -> 0
    m, x = torch.frexp(wf.abs().amax(dim=-1))
    e = torch.where(m > 0.75, x - 2, x - 3)
    e = torch.where(m == 0, torch.zeros_like(e), e).clamp(-MXFP4_EXP_MAX, MXFP4_EXP_MAX).to(torch.int32)
    scale = ((e + 127) << 23).view(torch.float32)  # 2^e exactly
    a = (wf / scale[..., None]).abs().clamp(max=MXFP4_MAX)  # a power-of-two division: exact
    # the grid's step is 0.5 below 2, 1 below 4, 2 above; torch.round takes ties to the even
    # multiple of the step, which is the even mantissa
    q = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2))
    lut = torch.tensor([0, 1, 2, 3, 4, 0, 5, 0, 6, 0, 0, 0, 7], dtype=torch.uint8, device=w.device)  # 2 value -> code
    c = lut[(q * 2).long()] | (torch.signbit(wf).to(torch.uint8) << 3)
    c = c.reshape(N, K // 2, 2)
    return c[..., 0] | (c[..., 1] << 4), (e + 127).to(torch.uint8)


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """(codes [N, K/2], scales [N, K/32]) -> [N, K]: code * 2^(scale - 127), exact in bf16 (an e2m1
    value has 2 significant bits)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    rows = max(1, _MXFP4_CHUNK // K)
    if N > rows:
        return torch.cat([dequantize_mxfp4(codes[i:i + rows], scales[i:i + rows], dtype) for i in range(0, N, rows)])
    c = torch.stack((codes & 15, codes >> 4), dim=-1).reshape(N, K).long()
    grid = torch.tensor(_E2M1_GRID + tuple(-v for v in _E2M1_GRID), dtype=torch.float32, device=codes.device)
    scale = (scales.to(torch.int32) << 23).view(torch.float32)
    return (grid[c].reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK) * scale[..., None]).reshape(N, K).to(dtype)


def pack_skinny_f4(codes: torch.Tensor, scales: torch.Tensor) -> tuple:
    """quantize_mxfp4's (codes [N, K/2], scales [N, K/32]) -> the layout gemm_dec's mxfp4 form
    streams: codes [N/16, K/128, 64, 16] bytes - block (n-tile j, k-step quad g) holds, for lane
    l = 16 q + r, four dwords, dword s the 8 codes W[16 j + r, 128 g + 32 s + 8 q : +8] (k-step
    4g + s, pack_skinny's fragment order): 1 KiB contiguous per block, four k-steps - and scales
    [N/16, K/128, 16, 4] bytes, dword (j, g, r) the e8m0 bytes of row 16 j + r for k-steps
    4g .. 4g + 3, the first in the low byte."""
    N, K = codes.shape[0], codes.shape[1] * 2
    if N % 16 or K % 128 or scales.shape != (N, K // MXFP4_BLOCK):
        raise ValueError(f"pack_skinny_f4: [{N}, {K}] needs N % 16 == 0, K % 128 == 0 and scales [N, K/32]")
    b = codes.contiguous().reshape(N // 16, 16, K // 128, 4, 4, 4).permute(0, 2, 4, 1, 3, 5)
    sp = scales.contiguous().reshape(N // 16, 16, K // 128, 4).permute(0, 2, 1, 3)
    return b.reshape(N // 16, K // 128, 64, 16).contiguous(), sp.contiguous()


def unpack_skinny_f4(cp: torch.Tensor, sp: torch.Tensor) -> tuple:
    nt, kg = cp.shape[0], cp.shape[1]
    b = cp.contiguous().reshape(nt, kg, 4, 16, 4, 4).permute(0, 3, 1, 4, 2, 5)
    s = sp.contiguous().reshape(nt, kg, 16, 4).permute(0, 2, 1, 3)
    return b.reshape(nt * 16, kg * 64).contiguous(), s.reshape(nt * 16, kg * 4).contiguous()


def is_mxfp4(w: Optional[torch.Tensor]) -> bool:
    """A weight in pack_skinny_f4's code layout (the only 4-d uint8 weight there is), or an
    [E, ...] stack of such (the only 5-d one)."""
    return w is not None and w.dtype == torch.uint8 and w.dim() in (4, 5)


def encode_weight(w: torch.Tensor, enc: str, gate_up8: bool = False, settle: bool = False) -> tuple:
    """THE encoding of a decode projection: the canonical row-major weight ``w`` [N, K] ->
    (the dequantised values [N, K] in ``w``'s dtype and row order, the packed codes, the packed
    scales) in the encoding ``enc`` ("fp8": quantize_rows_fp8 / pack_skinny_f8, scales [N] fp32;
    "mxfp4": quantize_mxfp4 / pack_skinny_f4).  ``gate_up8``: codes and scales in the
    [8 gate | 8 up] row order of the packed gate_up copy (interleave_gate_up8 - a row permutation,
    which per-row scales and per-row block scales follow).  ``settle``: the codes returned are those
    of the dequantised values, which is what encoding those values again reproduces: where a row's
    (block's) largest element rounded down to half the code range, the first pass's scale is one
    step coarser than the one the values themselves ask for - the same values on either."""
    if enc not in ("fp8", "mxfp4"):
        raise ValueError(f"encode_weight: encoding {enc!r}")
    f4 = enc == "mxfp4"
    quant, dequant = (quantize_mxfp4, dequantize_mxfp4) if f4 else (quantize_rows_fp8, dequantize_rows_fp8)
    q, s = quant(w)
    deq = dequant(q, s, w.dtype)
    if settle:
        q, s = quant(deq)
    if gate_up8 and f4:
        q, s = interleave_gate_up8(q), interleave_gate_up8(s)
    elif gate_up8:  # the row permutation moves bytes: through the uint8 view, the scales as a column
        q = interleave_gate_up8(q.view(torch.uint8)).view(torch.float8_e4m3fn)
        s = interleave_gate_up8(s[:, None])[:, 0]
    return (deq,) + (pack_skinny_f4(q, s) if f4 else (pack_skinny_f8(q), s.contiguous()))


def pack_skinny(w: torch.Tensor) -> torch.Tensor:
    """Row-major weight [N, K] -> the fragment-packed [N/16, K/32, 64, 8] layout of gemm_skinny:
    block (n-tile j, k-step s) holds, for lane l = 16 q + r, elements W[16 j + r, 32 s + 8 q : +8]
    (the v_mfma_f32_16x16x32_bf16 B operand), 1 KiB contiguous per block."""
    N, K = w.shape
    if N % 16 or K % 32:
        raise ValueError(f"pack_skinny: [{N}, {K}] needs N % 16 == 0 and K % 32 == 0")
    return w.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(N // 16, K // 32, 64, 8).contiguous()


def unpack_skinny(wp: torch.Tensor) -> torch.Tensor:
    nt, ks = wp.shape[0], wp.shape[1]
    return wp.reshape(nt, ks, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(nt * 16, ks * 32)


def interleave_gate_up(w13: torch.Tensor) -> torch.Tensor:
    """[gate (F rows); up (F rows)] -> per 128-row tile [64 gate | 64 up] rows (the SWIGLU
    epilogues: gate and up of an output column land in the same workgroup)."""
    F2, K = w13.shape
    F = F2 // 2
    if F % 64:
        raise ValueError("interleave_gate_up: F must be a multiple of 64")
    return w13.reshape(2, F // 64, 64, K).permute(1, 0, 2, 3).reshape(F2, K)


def deinterleave_gate_up(w: torch.Tensor) -> torch.Tensor:
    """Inverse of interleave_gate_up: per-128-row [64 gate | 64 up] -> [gate (F rows); up (F rows)]."""
    F2, K = w.shape
    return w.reshape(F2 // 128, 2, 64, K).permute(1, 0, 2, 3).reshape(F2, K)


# test / tool overrides (module attributes, not environment switches): a forced split-K factor for
# the slab-epilogue projections (real split-K slicing on tiny test shapes), and a forced waves-per-
# workgroup count for gemm_skinny (0 = the launcher's choice)
SKINNY_SPLITS_FORCE = 0
SKINNY_WAVES_FORCE = 0


def skinny_splits(N: int, K: int, target_wgs: int = 256) -> int:
    """Split-K factor for a slab-epilogue gemm_skinny: (N/64) x S workgroups ~ one per CU, each K
    slice at least 512 deep (tools/bench_skinny.py on MI355X, decode batch 1-64: S = 4 beats 2, 6
    and 8 for Llama-3-8B o/down - more slices add slab traffic to the reduce faster than they add
    weight-streaming parallelism).  ``SKINNY_SPLITS_FORCE`` (tests, tools) overrides."""
    if SKINNY_SPLITS_FORCE:
        return max(1, SKINNY_SPLITS_FORCE)
    tiles = max(1, N // 64)
    return max(1, min(K // 512, round(target_wgs / tiles)))


def skinny_workspace(max_m: int, N: int, splits: int, device) -> torch.Tensor:
    """fp32 split-K partial slabs [splits, max_m, N]."""
    return torch.empty(splits * min(max_m, SKINNY_MAX_M) * N, dtype=torch.float32, device=device)


def skinny_kchunk(K: int, S: int, rm: bool = False) -> int:
    """The K slice of each split (mirror of skinny_kchunk in csrc/gemm_skinny_plan.h, compared with
    it by tests/test_skinny_pack.py): rounded up to whole 128-deep wave groups where that keeps S
    slices, else to whole granules - 32-deep k-steps, or the 64-deep stages of the kernel over a
    row-major weight (``rm``)."""
    kc = -(-K // S)
    kc128 = -(-kc // 128) * 128
    if -(-K // kc128) == S:
        return kc128
    gran = 64 if rm else 32
    return -(-kc // gran) * gran


def skinny_nslabs(K: int, S: int, rm: bool = False) -> int:
    """The slabs a split-K launch with ``S`` splits writes: never more than S."""
    return -(-K // skinny_kchunk(K, S, rm))


# CPU forms of the skinny ops: the same packed layouts, split-K slicing and roundings as the
# kernels, so the decode control flow (and TP over gloo) is exercised by the CPU test suite.
def skinny_wdims(wp: torch.Tensor) -> tuple:
    """(N, K) of a skinny-GEMM weight: fragment-packed [N/16, K/32, 64, 8] or row-major [N, K]
    (the single resident copy, read by gemm_skinny_rm_kernel), or the fp8 decode encoding
    [N/16, K/64, 64, 16] (pack_skinny_f8), or the mxfp4 one [N/16, K/128, 64, 16] (pack_skinny_f4)."""
    if wp.dim() == 4:
        return wp.shape[0] * 16, wp.shape[1] * (128 if is_mxfp4(wp) else 64 if is_fp8(wp) else 32)
    return wp.shape[0], wp.shape[1]


def _cpu_w(wp: torch.Tensor, wscale: Optional[torch.Tensor] = None) -> torch.Tensor:
    if is_fp8(wp):  # the dequantised values, exactly the bf16 encoding's
        return unpack_skinny_f8(wp).float() * wscale.float()[:, None]
    if is_mxfp4(wp):
        return dequantize_mxfp4(*unpack_skinny_f4(wp, wscale), dtype=torch.float32)
    return (unpack_skinny(wp) if wp.dim() == 4 else wp).float()


def _cpu_deinterleave(gu: torch.Tensor) -> tuple:
    M, F2 = gu.shape
    t = gu.reshape(M, F2 // 128, 2, 64)
    return t[:, :, 0].reshape(M, F2 // 2), t[:, :, 1].reshape(M, F2 // 2)


def _rows(a: torch.Tensor, rows: Optional[int] = None) -> int:
    """Valid rows of an activation: row-major [M, K], or fragment-packed [ceil(M/16), K/32, 64, 8]
    (then ``rows`` must be given)."""
    if a.dim() == 4:
        if rows is None:
            raise ValueError("a fragment-packed activation needs its row count")
        return rows
    return a.shape[0]


def _cpu_a(a: torch.Tensor, rows: Optional[int]) -> torch.Tensor:
    return unpack_skinny(a)[: _rows(a, rows)] if a.dim() == 4 else a


def pack_activation(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row-major [M, K] -> fragment-packed [ceil(M/16), K/32, 64, 8] (rows padded with
    zeros), the A-operand layout gemm_skinny reads with whole-line loads."""
    M, K = x.shape
    mt = -(-M // 16)
    if M % 16:
        x = torch.cat([x, x.new_zeros(mt * 16 - M, K)])
    p = pack_skinny(x)
    return out.copy_(p) if out is not None else p


def _rn_scale(rownorm, M: int, K: int) -> Optional[torch.Tensor]:
    """CPU form of the deferred RMSNorm row scale: 1 / rms per row from partial sums of squares."""
    if rownorm is None:
        return None
    ss, eps = rownorm
    return torch.rsqrt(ss[:M].float().sum(1, keepdim=True) / K + eps)


def skinny_waves() -> int:
    """Waves per gemm_skinny workgroup: 0 = the launcher's choice (8 for split-K slabs, 4 for the
    single-slice epilogues); ``SKINNY_WAVES_FORCE`` = 4 or 8 forces one (tools)."""
    return SKINNY_WAVES_FORCE


def _rn_args(rownorm) -> tuple:
    return ((None, 0.0) if rownorm is None else (rownorm[0], float(rownorm[1]))) + (skinny_waves(),)


def skinny_auto_splits(M: int, N: int, K: int) -> int:
    """Mirror of skinny_auto_splits (csrc/gemm_skinny_plan.h): the largest power-of-two split that
    keeps the grid (64 columns per workgroup) within one workgroup per CU, K slices >= 512 deep
    and whole 256-deep rounds of the waves."""
    tiles = max(1, N // 64)
    sp = 1
    while sp < 16 and tiles * sp * 2 <= 256 and K // (sp * 2) >= 512 and K % (sp * 2 * 256) == 0:
        sp *= 2
    return sp


def skinny_linear(a: torch.Tensor, wp: torch.Tensor, out: Optional[torch.Tensor] = None,
                  nt_tiles: int = 4, rows: Optional[int] = None, rownorm: Optional[tuple] = None) -> torch.Tensor:
    """``a @ W^T`` for <= 64 rows over the fragment-packed weight, one K slice.  ``rownorm =
    (ss_part, eps)``: ``a`` holds x * norm_w (add_norm_partial) and the rows' 1/rms is applied to
    the outputs (the deferred RMSNorm)."""
    M = _rows(a, rows)
    if not _gpu(a):
        x = _cpu_a(a, rows)
        y = x.float() @ _cpu_w(wp).t()
        sc = _rn_scale(rownorm, M, x.shape[1])
        y = (y * sc if sc is not None else y).to(x.dtype)
        return out.copy_(y) if out is not None else y
    N = skinny_wdims(wp)[0]
    if out is None:
        out = torch.empty(M, N, dtype=a.dtype, device=a.device)
    native().gemm_skinny(a, wp, None, out, 1, 1, nt_tiles, M, *_rn_args(rownorm))
    return out


def skinny_swiglu(a: torch.Tensor, wp13: torch.Tensor, out: Optional[torch.Tensor] = None,
                  rows: Optional[int] = None, packed_out: bool = False,
                  rownorm: Optional[tuple] = None) -> torch.Tensor:
    """``silu(a @ Wg^T) * (a @ Wu^T)`` over a packed, gate/up-interleaved w13: [M, F], or with
    ``packed_out`` the fragment-packed [ceil(M/16), F/32, 64, 8] (the down projection's A)."""
    M = _rows(a, rows)
    F = skinny_wdims(wp13)[0] // 2
    if not _gpu(a):
        x = _cpu_a(a, rows)
        gu = x.float() @ _cpu_w(wp13).t()
        sc = _rn_scale(rownorm, M, x.shape[1])
        if sc is not None:
            gu = gu * sc
        g, u = _cpu_deinterleave(gu.to(x.dtype).float())
        y = (torch.nn.functional.silu(g) * u).to(x.dtype)
        if packed_out:
            y = pack_activation(y)
        return out.copy_(y) if out is not None else y
    if out is None:
        shape = (-(-M // 16), F // 32, 64, 8) if packed_out else (M, F)
        out = torch.empty(shape, dtype=a.dtype, device=a.device)
    native().gemm_skinny(a, wp13, None, out, 1, 3 if packed_out else 2, 4, M, *_rn_args(rownorm))
    return out


def skinny_slabs(a: torch.Tensor, wp: torch.Tensor, workspace: torch.Tensor, splits: int,
                 nt_tiles: int = 4, rows: Optional[int] = None, rownorm: Optional[tuple] = None) -> int:
    """Split-K ``a @ W^T`` into fp32 slabs [S', M, N] in ``workspace``; returns S'."""
    M = _rows(a, rows)
    if not _gpu(a):
        x = _cpu_a(a, rows)
        N, K = skinny_wdims(wp)
        if splits <= 0:
            splits = skinny_auto_splits(M, N, K)
        kc, ns = skinny_kchunk(K, splits, wp.dim() == 2), skinny_nslabs(K, splits, wp.dim() == 2)
        w = _cpu_w(wp)
        sc = _rn_scale(rownorm, M, K)
        slabs = workspace[: ns * M * N].view(ns, M, N)
        for s in range(ns):
            y = x[:, s * kc:(s + 1) * kc].float() @ w[:, s * kc:(s + 1) * kc].t()
            slabs[s] = y * sc if sc is not None else y
        return ns
    return native().gemm_skinny(a, wp, workspace, None, splits, 0, nt_tiles, M, *_rn_args(rownorm))


def skinny_grouped_swiglu(a: torch.Tensor, wp13: torch.Tensor, rows: int, out: Optional[torch.Tensor] = None
                          ) -> torch.Tensor:
    """MoE gate/up for every local expert in ONE launch (grid.z = experts): ``a`` is the shared
    fragment-packed activation [MT, K/32, 64, 8], ``wp13`` the stacked packed, gate/up-interleaved
    expert weights [E, 2F/16, K/32, 64, 8]; returns the per-expert packed SwiGLU activations
    [E, MT, F/32, 64, 8] (the grouped down projection's A)."""
    E, F = wp13.shape[0], skinny_wdims(wp13[0])[0] // 2
    mt = -(-rows // 16)
    if not _gpu(a):
        y = torch.stack([skinny_swiglu(a, wp13[e], rows=rows, packed_out=True) for e in range(E)])
        return out.copy_(y) if out is not None else y
    if out is None:
        out = torch.empty(E, mt, F // 32, 64, 8, dtype=a.dtype, device=a.device)
    native().gemm_skinny_grouped(a, wp13, None, out, 1, 3, rows, None, skinny_waves())
    return out


def skinny_grouped_slabs(act: torch.Tensor, wp2: torch.Tensor, workspace: torch.Tensor, rows: int,
                         row_w: torch.Tensor, splits: int = 1) -> int:
    """MoE down projection of every local expert in ONE launch: fp32 slabs [E * S', M, N] where
    expert e's rows are scaled by its routing weights ``row_w[:, e]`` (0 where not selected), so
    summing all slabs (add_norm_partial / reduce_slabs) IS the weighted expert combine.  Returns
    the slab count E * S'."""
    E, (N, K) = wp2.shape[0], skinny_wdims(wp2[0])
    M = rows
    if not _gpu(act):
        kc, ns = skinny_kchunk(K, splits, wp2.dim() == 3), skinny_nslabs(K, splits, wp2.dim() == 3)
        slabs = workspace[: E * ns * M * N].view(E * ns, M, N)
        for e in range(E):
            x = unpack_skinny(act[e])[:M].float()
            w = _cpu_w(wp2[e])
            for s in range(ns):
                slabs[e * ns + s] = (x[:, s * kc:(s + 1) * kc] @ w[:, s * kc:(s + 1) * kc].t()) * row_w[:M, e:e + 1]
        return E * ns
    return native().gemm_skinny_grouped(act, wp2, workspace, None, splits, 0, rows, row_w.contiguous(),
                                        skinny_waves())


# ---------------------------------------------------------------- decode GEMM, shared-A design (gemm_decode.hip)

def interleave_gate_up8(w13: torch.Tensor) -> torch.Tensor:
    """[gate (F rows); up (F rows)] -> per 16-row n-tile [8 gate | 8 up] rows: the DEC_SWIGLU8
    epilogue finds a feature's gate and up in lanes l and l ^ 8 of one accumulator."""
    F2, K = w13.shape
    F = F2 // 2
    if F % 8:
        raise ValueError("interleave_gate_up8: F must be a multiple of 8")
    return w13.reshape(2, F // 8, 8, K).permute(1, 0, 2, 3).reshape(F2, K)


def deinterleave_gate_up8(w: torch.Tensor) -> torch.Tensor:
    F2, K = w.shape
    return w.reshape(F2 // 16, 2, 8, K).permute(1, 0, 2, 3).reshape(F2, K)


# (splits, n-tiles per wave, waves, weight ring depth) per decode projection shape (N, K) at
# M <= 64: ~256 equal workgroups (measured: tools/bench_decode_gemm.py,
# profiles/r04/decode_gemm_sweep.jsonl).  Shapes not listed get an automatic pick.
# Round 24 (row-wide write-through slab stores, one split per XCD; same picks, same slabs;
# profiles/r24/launch_final_*.jsonl, M = 64 / M = 1 us against the parent in the same session):
# qkv 11.5 / 9.8 (12.7 / 9.8), o 9.2 / 7.2 (10.2 / 7.45), down 21.7 / 19.5 (22.9 / 20.3).
DEC_TABLE: dict = {
    # Llama-3-8B at TP=1 (profiles/r04/decode_gemm_sweep_v1.jsonl, M = 64 / M = 1 us):
    # qkv: 6 waves -> 64 column groups x 4 splits = 256 workgroups (8 waves left 64 CUs idle):
    # 12.1 vs 13.8 us at M = 64, 9.8 vs 11.0 at M = 1 (decode_gemm_qkv_6waves.jsonl)
    (6144, 4096, 0): (4, 1, 6, 8),      # qkv      12.1 / 9.8    (row-major skinny 13.5 / 10.6)
    (4096, 4096, 0): (8, 1, 8, 8),      # o         9.6 / 7.5    (10.2 / 7.5)
    (28672, 4096, 2): (1, 1, 7, 8),     # gate_up  39.9 / 38.1   (47.9 / 40.0)
    (4096, 14336, 0): (8, 1, 8, 8),     # down     22.3 / 19.0   (24.3 / 19.9)
    (128256, 4096, 1): (1, 4, 8, 4),    # LM head 173.8 / 166.0  (hipBLASLt 202.2 / 176.2)
    # Qwen3-8B (profiles/r21/dec_gemm_qwen3.jsonl, M = 64 / M = 1 us): its LM head's 9496 n-tiles
    # leave the rule's (1, 4, 8, 4) at 264.8 / 261.0 (4.70 / 4.77 TB/s, Llama's head: 6.16 / 6.40).
    # (1, 3, 8, 8) measured 228.8 / 204.9 but has no fp8 / mxfp4 instantiation; gate_up and down
    # stay on the rule's picks, Llama's (5.63 / 6.36 and 4.65 / 5.91 TB/s against 5.77 / 6.36 and 4.48 / 6.27)
    (151936, 4096, 1): (1, 2, 8, 8),    # LM head 234.3 / 205.3
}

# The same at 65..128 rows (the 5..8 m-tile instantiations of gemm_dec_kernel), from the sweep
# tools/bench_decode_gemm.py --ms 64,96,128 (profiles/r07/decode_gemm_m128_sweep.jsonl; us at
# M = 128 / 96 / 64 on one box).  The 64-row picks stay the fastest: fewer split-K slabs for o / down
# (half the slab bytes) lose more weight-streaming parallelism than they save - o (4, 1, 8, 8) 16.1
# and (4, 1, 4, 8) 15.0 us against 14.0, down 38.2 and 33.6 against 29.7; qkv on 8- or 4-wave
# workgroups 22.5 / 24.0 against 16.7.  The LM head takes two n-tiles per wave: 8 m-tiles x 4
# n-tiles of accumulators exceed the 256 registers of a wave at two waves per SIMD.
# Round 24 at M = 128 (profiles/r24): qkv 15.4 (17.2), o 12.9 (14.3), down 26.9 (30.2).
DEC_TABLE_M128: dict = {
    (6144, 4096, 0): (4, 1, 6, 8),      # qkv      16.7 / 14.7 / 12.6
    (4096, 4096, 0): (8, 1, 8, 8),      # o        14.0 / 11.8 / 10.2
    (28672, 4096, 2): (1, 1, 7, 8),     # gate_up  49.6 / 42.7 / 39.7
    (4096, 14336, 0): (8, 1, 8, 8),     # down     29.7 / 26.1 / 22.4
    (128256, 4096, 1): (1, 2, 8, 8),    # LM head 186.4 / 182.2 / 180.2 (hipBLASLt 223.7 / 214.1 / 205.5)
}


# fp8 weights: picks that differ from the bf16 tables' (keys as there plus the row class: 64 or
# 128).  A value of None routes the shape and row class to the bf16 encoding (dec_config answers
# None: not faster in fp8).  Empty: on the Llama-3-8B shapes and the 70B TP=1 gate_up, fp8 with the
# bf16 pick was the fastest in every row class, 1.13-2.05x over bf16 (profiles/r08/README.md).
DEC_TABLE_F8: dict = {}

# mxfp4 weights: the same, for the shapes that measure better on another pick of DEC_F4_FORMS or
# (None) on the bf16 copy.
DEC_TABLE_F4: dict = {}


# The SLAB epilogue and the split placement of gemm_dec_kernel (csrc/gemm_decode.hip), A/B only
# (module constants, not environment switches; -1 = as dec_slab_shipped routes, 0 = off, 1 = on
# wherever the launch can take it).  None of them changes a slab bit.
#   DEC_SLAB_ROWS   above 16 rows the accumulators are parked as rows in the dead A ring and stored
#                   as 16-byte pieces of whole rows (off, and up to 16 rows: one float per lane);
#   DEC_SLAB_WT     those 16-byte stores write through (sc1); only with DEC_SLAB_ROWS;
#   DEC_XCD_SPLITS  dense launches of 2, 4 or 8 splits whose workgroup count is a multiple of 8 deal
#                   one split to each XCD (dec_xcd_map), so an L2 fetches one A slice.
# They reach the kernel through native().gemm_dec; native().gemm_dec_plan reports what a launch does
# and dec_slab_plan mirrors it (tests/test_dec_slab_plan_cpu.py).
DEC_SLAB_ROWS = -1
DEC_SLAB_WT = -1
DEC_XCD_SPLITS = -1


def dec_slab_shipped(rows: int) -> tuple:
    """(rows, wt, xcd) as shipped for a SLAB launch of ``rows`` rows: dec_slab_shipped of
    csrc/gemm_dec_forms.h (from the A/B of profiles/r24/README.md) - all on above one m-tile; at
    one m-tile only the placement."""
    wide = int(rows > 16)
    return (wide, wide, 1)


def dec_xcd_ok(gx: int, splits: int) -> bool:
    return splits in (2, 4, 8) and (gx * splits) % 8 == 0


def dec_xcd_map(L: int, splits: int) -> tuple:
    """(column group, split) of the workgroup with linear id ``L`` = x + gx * y under the
    one-split-per-XCD placement: dec_xcd_map of csrc/gemm_dec_forms.h."""
    c, j, per = L % 8, L // 8, 8 // splits
    return j * per + c // splits, c % splits


def dec_slab_plan(M: int, N: int, cfg: tuple, grouped: bool = False, sw: Optional[tuple] = None) -> tuple:
    """(row-wide stores, write-through, one split per XCD) of a SLAB launch of ``cfg`` = (splits,
    ntw, waves, depth) at ``M`` rows over N columns: what dec_plan decides.  ``sw``: the three
    switches, default the module constants."""
    sr, sw_, sx = (DEC_SLAB_ROWS, DEC_SLAB_WT, DEC_XCD_SPLITS) if sw is None else sw
    S, ntw, waves, _ = cfg
    d = dec_slab_shipped(M)
    gx = -(-(N // 16) // (ntw * waves))
    rows = int((d[0] if sr < 0 else sr) != 0 and M > 16 and M * N * 4 < 0x7fffffff)
    wt = int(bool(rows) and (d[1] if sw_ < 0 else sw_) != 0)
    xcd = int((d[2] if sx < 0 else sx) != 0 and not grouped and dec_xcd_ok(gx, S))
    return rows, wt, xcd


def dec_config(N: int, K: int, epi: int, experts: int = 1, rows: int = 0, f8: bool = False,
               f4: bool = False) -> Optional[tuple]:
    """Launch configuration of gemm_dec for a weight [N, K]: (splits, ntw, waves, depth) or None
    when no configuration tiles the shape (the caller keeps gemm_skinny).  The candidates are the
    DEC_FORMS rows of the epilogue that serve ``rows``, in list order (the first of two equal
    candidates wins: (1, 4, 16) over (1, 4, 8) where both tile), without the table-only ones; split-K
    slabs try every form per split count.  Every Llama-3-8B / 70B / Mixtral projection and LM head
    at TP 1..8 picks one of them (tools/bench_decode_gemm.py passes ``cfg`` to dec_gemm to time
    others).  ``experts`` > 1: a grouped launch (grid.z = expert), whose
    workgroup count is per expert times experts (Mixtral down: 32 column groups x 8 experts, no
    split - the expert slabs are the split).  ``rows`` > 64 (dense launches only, up to
    DEC_MAX_M): the pick among the forms instantiated with 5..8 m-tiles; ``rows`` <= 64 (or not
    given) never changes the answer.  ``f8``: the configuration over the fp8 encoding of the
    weight (dense launches, K a multiple of 64) - the same tables and candidates restricted to
    DEC_F8_FORMS, DEC_TABLE_F8 first; None where the shape decodes from bf16.  ``f4``: the same over
    the mxfp4 encoding (K a multiple of 128, DEC_F4_FORMS, DEC_TABLE_F4; every K slice whole
    256-deep A chunks).  Grouped launches over a quantised stack have a rule of their own,
    dec_grouped_q_config: ``f8`` / ``f4`` with ``experts`` != 1 answers None here."""
    if (f8 or f4) and experts != 1:  # the quantised grouped launches answer to dec_grouped_q_config
        return None
    return _dec_pick(N, K, epi, experts, rows, f8, f4)


def _dec_pick(N: int, K: int, epi: int, experts: int, rows: int, f8: bool, f4: bool) -> Optional[tuple]:
    """dec_config's rule (tables, then the candidate walk), whatever the expert count."""
    wide = rows > DEC_NARROW_MAX_M
    if wide and (experts != 1 or rows > DEC_MAX_M):
        return None
    if f8 and K % 64:
        return None
    if f4 and (f8 or K % 128):
        return None
    compiled = ([DEC_FORMS[i] for i in DEC_F8_FORMS] if f8 else
                [DEC_FORMS[i] for i, _ in DEC_F4_FORMS] if f4 else DEC_FORMS)
    if f8 and experts == 1 and (N, K, epi, 128 if wide else 64) in DEC_TABLE_F8:
        return DEC_TABLE_F8[(N, K, epi, 128 if wide else 64)]
    if f4 and experts == 1 and (N, K, epi, 128 if wide else 64) in DEC_TABLE_F4:
        return DEC_TABLE_F4[(N, K, epi, 128 if wide else 64)]
    hit = (DEC_TABLE_M128 if wide else DEC_TABLE).get((N, K, epi)) if experts == 1 else None
    if hit is not None and (not f8 or dec_form_ok(epi, hit, rows, f8=True)) and (
            not f4 or dec_form_ok(epi, hit, rows, f4=True, K=K)):
        return hit
    ntiles, ksteps = N // 16, K // 32
    forms = [f[1:4] for f in compiled
             if f[0] == epi and rows <= 16 * f[4] and f[:4] not in DEC_FORMS_TABLE_ONLY]
    cands = [(s,) + f for s in ((1, 2, 4, 8, 16) if epi == DEC_SLAB else (1,)) for f in forms]
    best = None
    for s, ntw, w, d in cands:
        if experts > 1 and s > 1:  # grouped: the per-expert slabs are the split (workspace E x M x N)
            continue
        it = 8 if f4 else max(d, 8)  # mxfp4: the launcher fits the ring depth to the slice
        if (epi == 0 and ntiles % (ntw * w)) or K % s or (ksteps // s) % it or ksteps % s:
            continue
        wgs = -(-ntiles // (ntw * w)) * s * experts
        # ~256 workgroups; for split-K slabs 8-wave workgroups of one n-tile per wave were the
        # fastest within 64 workgroups of that (the sweep), then fewer K splits (slab traffic)
        far = abs(wgs - 256) if wgs <= 512 else 10_000 + wgs
        key = ((far > 64, -w, far, s) if epi == 0 else (far, s))
        if best is None or key < best[0]:
            best = (key, (s, ntw, w, d))
    return best[1] if best else None


def dec_available(N: int, K: int, epi: int, rows: int = 0) -> bool:
    return dec_config(N, K, epi, rows=rows) is not None


# Quantised grouped launches: (N, K, epi, experts, "fp8" | "mxfp4") -> a pick that differs from the
# rule's, or None to route the projection of that many local experts to the bf16 stacks
# (dec_grouped_q_config answers None: not faster than bf16).  Measurements: profiles/r14/README.md.
DEC_TABLE_GROUPED_Q: dict = {}


def dec_grouped_q_config(N: int, K: int, epi: int, experts: int, f8: bool = False, f4: bool = False) -> Optional[tuple]:
    """Launch configuration (splits, ntw, waves, depth) of a grouped gemm_dec (grid.z = expert,
    <= DEC_NARROW_MAX_M rows) over the fp8 (``f8``) or mxfp4 (``f4``) encoding of an expert stack
    [experts, N, K], or None where the stack decodes from bf16: dec_config's rule with the
    candidates restricted to DEC_F8_FORMS / DEC_F4_FORMS - splits 1 when ``experts`` > 1 (the expert
    slabs are the split), K a multiple of 64 (fp8) or of 128 with whole 256-deep K slices (mxfp4) -
    behind DEC_TABLE_GROUPED_Q.  SLAB and SWIGLU8 epilogues only."""
    if f8 == f4 or experts < 1 or epi not in (DEC_SLAB, DEC_SWIGLU8):
        return None
    key = (N, K, epi, experts, "mxfp4" if f4 else "fp8")
    if key in DEC_TABLE_GROUPED_Q:
        return DEC_TABLE_GROUPED_Q[key]
    return _dec_pick(N, K, epi, experts, 0, f8, f4)


def dec_grouped_q_form_ok(epi: int, cfg: tuple, rows: int, f8: bool = False, f4: bool = False, K: int = 0) -> bool:
    """Whether gemm_decode.hip has an instantiation for a grouped launch of
    ``cfg = (splits, ntw, waves, depth)`` at ``rows`` rows over fp8 (``f8``) or mxfp4 (``f4``)
    codes: a SLAB or SWIGLU8 row of DEC_F8_FORMS / DEC_F4_FORMS, at most DEC_NARROW_MAX_M rows; mxfp4
    with ``K`` given: every K slice whole 256-deep A chunks."""
    if f8 == f4 or rows > DEC_NARROW_MAX_M or epi not in (DEC_SLAB, DEC_SWIGLU8):
        return False
    return dec_form_ok(epi, cfg, rows, f8=f8, f4=f4, K=K)


def grouped_q_wdims(wq: torch.Tensor) -> tuple:
    """(E, N, K) of a quantised expert stack: fp8 codes [E, N/16, K/64, 64, 16] or mxfp4 codes
    [E, N/16, K/128, 64, 16]."""
    if wq.dim() != 5 or not (is_fp8(wq) or is_mxfp4(wq)) or tuple(wq.shape[3:]) != (64, 16):
        raise ValueError("a quantised expert stack is float8_e4m3fn [E, N/16, K/64, 64, 16] or uint8 "
                         f"[E, N/16, K/128, 64, 16], not {wq.dtype} {tuple(wq.shape)}")
    return wq.shape[0], wq.shape[1] * 16, wq.shape[2] * (128 if is_mxfp4(wq) else 64)


def enc_kw(x) -> dict:
    """dec_config's / dec_form_ok's keyword for a quantised encoding: ``x`` its name ("fp8" |
    "mxfp4") or a codes tensor, which says which encoding it is."""
    if x == "mxfp4" or (isinstance(x, torch.Tensor) and is_mxfp4(x)):
        return {"f4": True}
    if x == "fp8" or (isinstance(x, torch.Tensor) and is_fp8(x)):
        return {"f8": True}
    raise ValueError(f"not a quantised decode encoding: {x if isinstance(x, str) else x.dtype}")


def is_codes(w: Optional[torch.Tensor]) -> bool:
    """A weight held as a quantised decode encoding's packed codes (fp8 or mxfp4)."""
    return is_fp8(w) or is_mxfp4(w)


def enc_name(w: Optional[torch.Tensor]) -> str:
    """"fp8" | "mxfp4" for a codes tensor, "bf16" for anything else (None included)."""
    return "mxfp4" if is_mxfp4(w) else "fp8" if is_fp8(w) else "bf16"


def dequantize_codes(w: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """Packed codes (pack_skinny_f8 with row scales, or pack_skinny_f4 with packed block scales) ->
    the row-major [N, K] values in the codes' row order: exactly what they were quantised from."""
    if is_mxfp4(w):
        return dequantize_mxfp4(*unpack_skinny_f4(w, scale), dtype=dtype)
    return dequantize_rows_fp8(unpack_skinny_f8(w), scale, dtype)


def _dec_gemm(name: str, a: torch.Tensor, w: torch.Tensor, wscale: Optional[torch.Tensor], epi: int, rows: int,
              workspace: Optional[torch.Tensor], out: Optional[torch.Tensor], rownorm: Optional[tuple],
              row_w: Optional[torch.Tensor], cfg: Optional[tuple], E: int, delta: Optional[tuple] = None) -> int:
    """The one body of dec_gemm (``E`` = 0), dec_gemm_grouped and dec_gemm_grouped_q (``E`` experts,
    ``w`` and ``wscale`` [E, ...] stacks): checks, configuration, the CPU reference - one per-expert
    loop with the kernel's split-K slicing over the dequantised values - and the one native launch."""
    f8, f4 = is_fp8(w), is_mxfp4(w)
    enc = "mxfp4" if f4 else "fp8" if f8 else None
    N, K = skinny_wdims(w[0] if E else w)
    M = rows
    lead = (E,) if E else ()
    want = lead + ((N // 16, K // 128, 16, 4) if f4 else (N,))
    if enc and (wscale is None or (wscale.numel() != N if f8 and not E else
                                   tuple(wscale.shape) != want or wscale.dtype != (torch.uint8 if f4 else torch.float32))):
        raise ValueError(f"{name}: the {enc} {'stack' if E else 'weight'} needs its scales {list(want)} "
                         + ("uint8 (the packed block scales)" if f4 else "fp32"))
    limit = DEC_NARROW_MAX_M if E and enc else DEC_MAX_M
    if M > limit and (enc or not E or not _gpu(a)):  # (a bf16 stack on the GPU: the form check below refuses)
        raise ValueError(f"{name}: at most {limit} rows, got {M}")
    if E and enc and epi not in (DEC_SLAB, DEC_SWIGLU8):
        raise ValueError(f"{name}: only the slab and SwiGLU epilogues")
    if cfg is None:
        cfg = (dec_grouped_q_config(N, K, epi, E, **enc_kw(w)) if E and enc else
               dec_config(N, K, epi, experts=E) if E else dec_config(N, K, epi, rows=M, f8=f8, f4=f4))
    if cfg is None:
        raise ValueError(f"{name}: no configuration for N={N} K={K} epi={epi} " + (f"experts={E}" if E else f"rows={M}"))
    S, ntw, waves, depth = cfg
    if delta is not None:
        dl, dslot, dn = delta
        if epi != DEC_SWIGLU8 or E:
            raise ValueError(f"{name}: a pre-activation delta goes with the SwiGLU epilogue of a dense launch only")
        if rownorm is not None and rownorm[0].shape[1] > 16:
            raise ValueError(f"{name}: a delta goes with at most 16 deferred-norm sums per row")
        if dl.dtype != torch.float32 or dl.numel() < M * N or dslot is None or dslot.numel() < M or dn < 1:
            raise ValueError(f"{name}: delta must be fp32 [{M}, {N}] with delta_slot [{M}] and delta_slots >= 1")
    if not _gpu(a):
        sc = _rn_scale(rownorm, M, K)
        for e in range(max(E, 1)):
            x = _cpu_a(a[e] if a.dim() == 5 else a, rows).float()
            wf = _cpu_w(w[e], wscale[e] if enc else None) if E else _cpu_w(w, wscale)
            if epi == 0:
                kc = K // S
                slabs = workspace[e * S * M * N: (e + 1) * S * M * N].view(S, M, N)
                for s in range(S):
                    y = x[:, s * kc:(s + 1) * kc] @ wf[:, s * kc:(s + 1) * kc].t()
                    slabs[s] = y * sc if sc is not None else y
                if row_w is not None:
                    slabs.mul_(row_w[:M, e].float().view(1, M, 1))
                continue
            y = x @ wf.t()
            if sc is not None:
                y = y * sc
            if delta is not None:  # packed order, after the row scale, before any rounding
                on = ((dslot[:M] >= 0) & (dslot[:M] < dn)).nonzero().flatten()
                y[on] = y[on] + dl.reshape(-1)[:M * N].view(M, N)[on].float()
            o = out[e] if E else out
            if epi == 1:
                o[:M].copy_(y.to(o.dtype))
            else:
                gu = deinterleave_gate_up8(y.to(a.dtype).float().t()).t()
                g, u = gu[:, : N // 2], gu[:, N // 2:]
                o.copy_(pack_activation((torch.nn.functional.silu(g) * u).to(a.dtype)))
        return max(E, 1) * S if epi == 0 else 1
    rn = (None, 0.0) if rownorm is None else (rownorm[0], float(rownorm[1]))
    # more than 16 partial sums per row: gemm_dec_rc's per-16-column sums, the wide-norm form
    wn = rownorm is not None and rownorm[0].shape[1] > 16
    ok = (dec_grouped_q_form_ok(epi, cfg, M, K=K, **enc_kw(w)) if E and enc else
          dec_form_ok(epi, cfg, M, grouped=E > 0, wide_norm=wn, f8=f8, f4=f4, K=K))
    if not ok:
        raise RuntimeError(f"{name}: form (epi, ntw, waves, depth) = {(epi,) + tuple(cfg[1:])} not compiled for "
                           f"{M} rows" + (" of a grouped launch" if E else "") +
                           (" with the wide deferred norm" if wn else "") +
                           (" over fp8 weights" if f8 else f" over mxfp4 weights in {S} K slices" if f4 else ""))
    r = native().gemm_dec(a, w, wscale if enc else None, workspace, out, S, epi, ntw, waves, depth, M, *rn,
                          row_w if E else None, DEC_F4_DEPTH_FORCE if f4 else 0, DEC_SLAB_ROWS, DEC_SLAB_WT,
                          DEC_XCD_SPLITS, *((dl, dslot, dn) if delta is not None else ()))
    if r < 0:
        raise RuntimeError(f"{name}: configuration {cfg} not compiled for N={N} K={K} epi={epi}")
    return r


def dec_gemm(a: torch.Tensor, wp: torch.Tensor, epi: int, rows: int, workspace: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, rownorm: Optional[tuple] = None,
             cfg: Optional[tuple] = None, wscale: Optional[torch.Tensor] = None,
             delta: Optional[torch.Tensor] = None, delta_slot: Optional[torch.Tensor] = None,
             delta_slots: int = 0) -> int:
    """gemm_dec over a fragment-packed activation ``a`` and packed weight ``wp`` (pack_skinny: under
    ONE_LAYOUT the model's only copy, which prefill's tile GEMM reads too; else a copy for decode).
    epi 0: fp32 split-K slabs into ``workspace`` [S, M, N], returns S; epi 1: ``out`` [M, N] bf16;
    epi 2: ``out`` packed SwiGLU [ceil(M/16), F/32, 64, 8] over an interleave_gate_up8 weight.
    ``rownorm = (ss_part, eps)``: deferred RMSNorm of the A rows (add_norm_partial).  Up to
    DEC_MAX_M = 128 rows; the configuration is dec_config's for that row count (65..128 rows run
    the 5..8 m-tile instantiations).  ``wp`` may be the fp8 encoding (pack_skinny_f8 codes) with
    ``wscale`` its per-row scales in packed row order: the same launch over half the weight
    bytes, bit-identical to the bf16 launch of the same configuration over the dequantised
    weights; a form without an fp8 instantiation raises.  Or the mxfp4 encoding (pack_skinny_f4's
    codes, ``wscale`` its packed block scales), under the same contract.
    ``delta`` (epi 2 only): fp32 [M, N] over the packed row index (column n belongs to packed weight
    row n - what ``lora_slab(.., "w13", ..)`` writes), added to the accumulator of the rows whose
    ``delta_slot[row]`` (int32) lies in ``[0, delta_slots)`` after the deferred-norm and fp8 row
    scales and before gate and up are rounded to bf16; the other rows compute exactly what a launch
    without delta computes.  Not with more than 16 deferred-norm sums per row.
    CPU: the fp32 reference with the same split-K slicing (over the dequantised values)."""
    dl = None if delta is None else (delta, delta_slot, int(delta_slots))
    return _dec_gemm("gemm_dec", a, wp, wscale, epi, rows, workspace, out, rownorm, None, cfg, 0, delta=dl)


def dec_gemm_grouped(a: torch.Tensor, wp: torch.Tensor, epi: int, rows: int, workspace: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, row_w: Optional[torch.Tensor] = None,
                     cfg: Optional[tuple] = None) -> int:
    """gemm_dec over every local expert of a MoE layer in ONE launch (grid.z = expert): ``wp``
    [E, N/16, K/32, 64, 8] (packed per expert, gate/up interleave_gate_up8 for epi 2); ``a`` packed
    [ceil(M/16), K/32, 64, 8] shared by the experts (gate_up) or [E, ...] per expert (down).
    epi 2: ``out`` [E, ceil(M/16), F/32, 64, 8] packed SwiGLU; epi 0: fp32 slabs [E * S, M, N] in
    ``workspace`` scaled by ``row_w`` [M, E] (routing weights, 0 where a row skipped the expert),
    returns E * S - the residual-add kernel's slab sum is the expert combine."""
    if wp.dtype == torch.uint8:
        raise ValueError("gemm_dec_grouped: grouped launches have no mxfp4 form here (dec_gemm_grouped_q takes the "
                         "codes with their scales)")
    return _dec_gemm("gemm_dec_grouped", a, wp, None, epi, rows, workspace, out, None, row_w, cfg, wp.shape[0])


def dec_gemm_grouped_q(a: torch.Tensor, wq: torch.Tensor, wqs: torch.Tensor, epi: int, rows: int,
                       workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                       row_w: Optional[torch.Tensor] = None, cfg: Optional[tuple] = None) -> int:
    """dec_gemm_grouped over the quantised encoding of the expert stack: ``wq`` the fp8 codes
    [E, N/16, K/64, 64, 16] with ``wqs`` [E, N] fp32 row scales in packed row order (pack_skinny_f8 /
    quantize_rows_fp8 per expert), or the mxfp4 codes [E, N/16, K/128, 64, 16] with ``wqs`` the packed
    block scales [E, N/16, K/128, 16, 4] uint8 (pack_skinny_f4 per expert).  ``a``, ``out``,
    ``workspace`` and ``row_w`` as dec_gemm_grouped; the configuration is dec_grouped_q_config's.
    One launch over half (a quarter of) the weight bytes, bit-identical to dec_gemm_grouped of the
    same configuration over the dequantised stack."""
    E = grouped_q_wdims(wq)[0]  # raises for anything but a stack of codes
    return _dec_gemm("gemm_dec_grouped_q", a, wq, wqs, epi, rows, workspace, out, None, row_w, cfg, E)


def dec_gemm_rc(a: torch.Tensor, wp: torch.Tensor, rows: int, residual: torch.Tensor, norm_w: torch.Tensor,
                eps: float) -> Optional[tuple]:
    """Row-complete decode GEMM (gemm_dec_rc_kernel) for a residual-producing projection:
    ``residual += a . W^T`` in place (no split-K slabs) and the next GEMM's deferred-RMSNorm
    operands in the same launch: returns ``(xw, (ss, eps))`` - xw = residual * norm_w
    fragment-packed, ss [rows, N/16] per-16-column sums of squares - or None where the kernel does
    not tile the shape (the caller keeps slabs + add_norm_partial).  CPU: the fp32 reference with
    the same 8 K-slices summed in slice order."""
    N, K = skinny_wdims(wp)
    M = rows
    if K % 256 or N % 32 or M > 64:
        return None
    xw = packed_empty(M, N, residual.dtype, residual.device)
    ss = torch.empty(M, N // 16, dtype=torch.float32, device=residual.device)
    if not _gpu(a):
        x = _cpu_a(a, rows).float()
        w = _cpu_w(wp)
        kc = K // 8
        h = residual[:M].float()
        for s in range(8):
            h = h + x[:, s * kc:(s + 1) * kc] @ w[:, s * kc:(s + 1) * kc].t()
        residual[:M] = h.to(residual.dtype)
        v = residual[:M].float()
        ss.copy_((v * v).view(M, N // 16, 16).sum(-1))
        xw.copy_(pack_activation((v * norm_w.float()).to(residual.dtype)))
        return xw, (ss, eps)
    if not native().gemm_dec_rc(a, wp, residual, norm_w, xw, ss, rows):
        return None
    return xw, (ss, eps)


def add_norm_partial(residual: torch.Tensor, workspace: Optional[torch.Tensor], nslabs: int, norm_w: torch.Tensor,
                     out: Optional[torch.Tensor] = None, ss_part: Optional[torch.Tensor] = None,
                     packed: bool = True) -> tuple:
    """Residual update with a deferred RMSNorm: ``residual <- residual + sum of slabs``;
    returns ``(residual * norm_w`` (fragment-packed by default), ``ss_part [M, d/512])`` for a
    consumer skinny GEMM called with ``rownorm=(ss_part, eps)``.  One wave per 512 columns: the
    norm's row reduction is left to the consumer's epilogue."""
    M, d = residual.shape
    if ss_part is None:
        ss_part = torch.empty(M, d // 512, dtype=torch.float32, device=residual.device)
    if out is None:
        out = packed_empty(M, d, residual.dtype, residual.device) if packed else torch.empty_like(residual)
    if not _gpu(residual):
        if nslabs:
            s = workspace[: nslabs * M * d].view(nslabs, M, d).sum(0)
            residual.copy_((residual.float() + s).to(residual.dtype))
        v = residual.float()
        ss_part.copy_((v * v).view(M, d // 512, 512).sum(-1))
        y = (v * norm_w.float()).to(residual.dtype)
        out.copy_(pack_activation(y) if out.dim() == 4 else y)
        return out, ss_part
    native().add_norm_partial(out, residual, workspace, nslabs, norm_w, ss_part)
    return out, ss_part


def reduce_slabs(workspace: torch.Tensor, nslabs: int, M: int, N: int, dtype=torch.bfloat16,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sum of ``nslabs`` split-K slabs [nslabs, M, N] -> [M, N] in ``dtype`` (TP>1 tails, before
    the all-reduce)."""
    if not _gpu(workspace):
        y = workspace[: nslabs * M * N].view(nslabs, M, N).sum(0).to(dtype)
        return out.copy_(y) if out is not None else y
    if out is None:
        out = torch.empty(M, N, dtype=dtype, device=workspace.device)
    native().reduce_slabs(out, workspace, nslabs)
    return out


def reduce_add_rms_norm(out: torch.Tensor, residual: torch.Tensor, workspace: Optional[torch.Tensor], nslabs: int,
                        norm_w: torch.Tensor, eps: float, packed_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``residual <- residual + sum of slabs`` (rounded to the residual dtype), ``out <- rms_norm``.
    ``nslabs = 0``: a plain RMSNorm of ``residual``.  A 4-D ``out`` is written fragment-packed
    ([ceil(M/16), d/32, 64, 8], the next skinny GEMM's A operand); ``packed_out``: a second,
    packed copy of the same rows (same launch)."""
    if not _gpu(residual):
        M, N = residual.shape
        if nslabs:
            s = workspace[: nslabs * M * N].view(nslabs, M, N).sum(0)
            residual.copy_((residual.float() + s).to(residual.dtype))
        y = ref.rms_norm(residual, norm_w, eps)
        if packed_out is not None:
            packed_out.copy_(pack_activation(y))
        return out.copy_(pack_activation(y) if out.dim() == 4 else y)
    native().reduce_add_rms_norm(out, residual, workspace, nslabs, norm_w, eps, packed_out)
    return out


def packed_empty(M: int, K: int, dtype, device) -> torch.Tensor:
    """Uninitialised fragment-packed activation buffer [ceil(M/16), K/32, 64, 8]."""
    return torch.empty(-(-M // 16), K // 32, 64, 8, dtype=dtype, device=device)


# ---------------------------------------------------------------- per-request LoRA adapters

# the adapted projections: the fused qkv is one of them, and so is the fused gate_up ("w13": its B
# rows in the row order of the model's resident w13, so the delta's column n is packed weight row n)
LORA_PROJ = ("wqkv", "wo", "w2", "w13")
LORA_RANK_ALIGN = 32  # rank capacities are whole r-steps of lora_expand_kernel
LORA_MAX_CAP = 224  # kernel limit of a projection's rank capacity (the expand kernel's LDS image of t)


class LoraState:
    """The device arena of the resident low-rank adapters (csrc/lora.hip), one slot per adapter.

    Per adapted projection ``p`` of ``LORA_PROJ`` with shape ``dims[p] = (N, K, R)``: ``A[p]``
    ``[layers, slots, R, K]`` and ``B[p]`` ``[layers, slots, N, R]`` in ``dtype`` (bf16 on the GPU),
    zero where an adapter has a smaller rank or lacks the target; ``scaling`` fp32 ``[slots]``
    (``lora_alpha / r``, or ``/ sqrt(r)`` with rslora).  ``R`` is the projection's rank capacity, a
    multiple of ``LORA_RANK_ALIGN``.  A step's row names its slot through ``ops.lora_slab`` /
    ``ops.lora_add`` (``slot`` int32, -1 = no adapter)."""

    def __init__(self, slots: int, layers: int, dims: dict, device, dtype=torch.bfloat16):
        self.slots, self.layers = int(slots), int(layers)
        if self.slots <= 0 or self.layers <= 0:
            raise ValueError("a LoRA state needs slots and layers")
        self.dims, self.dtype = {}, dtype
        self.A, self.B = {}, {}
        dev = torch.device(device)
        for p, (N, K, R) in dims.items():
            if p not in LORA_PROJ:
                raise ValueError(f"LoRA: {p!r} is not an adapted projection {LORA_PROJ}")
            R = -(-int(R) // LORA_RANK_ALIGN) * LORA_RANK_ALIGN
            if R > LORA_MAX_CAP:
                raise ValueError(f"LoRA: rank capacity {R} of {p} exceeds the kernels' {LORA_MAX_CAP}")
            if dev.type == "cuda" and (N % 16 or K % 32):
                raise ValueError(f"LoRA: {p} [{N}, {K}] needs N % 16 == 0 and K % 32 == 0")
            self.dims[p] = (int(N), int(K), R)
            self.A[p] = torch.zeros(self.layers, self.slots, R, K, dtype=dtype, device=dev)
            self.B[p] = torch.zeros(self.layers, self.slots, N, R, dtype=dtype, device=dev)
        self.scaling = torch.zeros(self.slots, dtype=torch.float32, device=dev)
        self.device = self.scaling.device

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (*self.A.values(), *self.B.values(), self.scaling))

    def set_scaling(self, slot: int, scaling: float) -> None:
        self.scaling[slot] = float(scaling)

    def load(self, slot: int, layer: int, proj: str, A: torch.Tensor, B: torch.Tensor,
             r0: int = 0, n0: int = 0) -> None:
        """Adapter ``slot``'s pair of ``(layer, proj)``: ``A`` [r, K] into rank rows ``[r0, r0 + r)``
        and ``B`` [n, r] into output rows ``[n0, n0 + n)`` of the same rank columns - the fused qkv
        takes q, k and v at rank offsets 0, cap, 2 cap and their output ranges (B block-diagonal)."""
        if not 0 <= slot < self.slots:
            raise ValueError(f"slot {slot} outside [0, {self.slots})")
        N, K, R = self.dims[proj]
        r = A.shape[0]
        if A.shape[1] != K or B.shape[1] != r or r0 + r > R or n0 + B.shape[0] > N:
            raise ValueError(f"LoRA {proj}: A {list(A.shape)} / B {list(B.shape)} do not fit [{N}, {K}] at rank "
                             f"capacity {R} (rank offset {r0}, row offset {n0})")
        self.A[proj][layer, slot, r0:r0 + r] = A.to(self.device, self.dtype)
        self.B[proj][layer, slot, n0:n0 + B.shape[0], r0:r0 + r] = B.to(self.device, self.dtype)


def lora_shrink_plan(K: int) -> int:
    """K slices S of a lora_shrink launch (``t_part`` [S, M, R]); mirror of k8sllm_lora_shrink_plan,
    which the binding reports (compared by tests/test_lora_gpu.py)."""
    nk = K // 32
    s0 = min(16, max(1, K // 512))
    per = -(-nk // s0)
    return -(-nk // per)


def _lora_t(state: "LoraState", layer: int, proj: str, x: torch.Tensor, rows: int, slot: torch.Tensor,
            rownorm: Optional[tuple]) -> tuple:
    """lora_shrink launch: (t_part [S, M, R] fp32, S)."""
    N, K, R = state.dims[proj]
    S = lora_shrink_plan(K)
    t_part = torch.empty(S * rows * R, dtype=torch.float32, device=x.device)
    ss, eps = (None, 0.0) if rownorm is None else (rownorm[0], float(rownorm[1]))
    used = native().lora_shrink(x, state.A[proj][layer], slot, t_part, rows, ss, eps)
    if used != S:
        raise RuntimeError(f"lora_shrink: the kernel used {used} K slices, the plan says {S}")
    return t_part, S


def lora_slab(state: "LoraState", layer: int, proj: str, a: torch.Tensor, rows: int, workspace: torch.Tensor,
              ns: int, slot: torch.Tensor, rownorm: Optional[tuple] = None) -> int:
    """One more split-K slab for a decode projection: slab ``ns`` of ``workspace`` ([.., rows, N] fp32)
    ``= scaling[s] * B[s] (A[s] a[row])`` for rows with ``s = slot[row] >= 0``, exact zeros for the
    others; returns ``ns + 1``.  ``a``: the projection's A operand, fragment-packed with ``rows``
    valid rows or row-major; ``rownorm = (ss_part, eps)``: its deferred RMSNorm, as the GEMM got it.
    CPU: ``ref.lora_delta`` in fp32."""
    N, K, R = state.dims[proj]
    M = _rows(a, rows)
    if workspace.numel() < (ns + 1) * M * N:
        raise ValueError(f"lora_slab: the workspace has no room for slab {ns} of [{M}, {N}]")
    if not _gpu(a):
        x = _cpu_a(a, rows)
        d = ref.lora_delta(x, state.A[proj][layer], state.B[proj][layer], state.scaling, slot)
        sc = _rn_scale(rownorm, M, K)
        workspace[ns * M * N:(ns + 1) * M * N].view(M, N).copy_(d * sc if sc is not None else d)
        return ns + 1
    t_part, S = _lora_t(state, layer, proj, a, M, slot, rownorm)
    native().lora_expand(t_part, S, state.B[proj][layer], state.scaling, slot, workspace, M, ns)
    return ns + 1


def lora_add(state: "LoraState", layer: int, proj: str, x: torch.Tensor, y: torch.Tensor, slot: torch.Tensor
             ) -> torch.Tensor:
    """``y[row] <- dtype(float(y[row]) + scaling[s] * B[s] (A[s] x[row]))`` in place for rows with
    ``s = slot[row] >= 0``; the other rows are not touched.  ``x`` [M, K], ``y`` [M, N] row-major.
    CPU: ``ref.lora_delta`` in fp32."""
    M = x.shape[0]
    if y.shape[0] != M or y.shape[1] != state.dims[proj][0] or x.shape[1] != state.dims[proj][1]:
        raise ValueError(f"lora_add: x {list(x.shape)} / y {list(y.shape)} do not match {proj} {state.dims[proj][:2]}")
    if M == 0:
        return y
    if not _gpu(x):
        d = ref.lora_delta(x, state.A[proj][layer], state.B[proj][layer], state.scaling, slot)
        on = (slot[:M] >= 0).nonzero().flatten()
        y[on] = (y[on].float() + d[on]).to(y.dtype)
        return y
    t_part, S = _lora_t(state, layer, proj, x, M, slot, None)
    native().lora_expand(t_part, S, state.B[proj][layer], state.scaling, slot, y, M, -1)
    return y


def proj_add_rms_norm(a: torch.Tensor, wp: torch.Tensor, residual: torch.Tensor, norm_w: torch.Tensor, eps: float,
                      workspace: Optional[torch.Tensor] = None, splits: Optional[int] = None,
                      out: Optional[torch.Tensor] = None, rows: Optional[int] = None,
                      packed_out: bool = False) -> torch.Tensor:
    """The decode tail of an attention or MLP block in one GEMM + one reduce:
    ``residual <- residual + a @ W^T``; returns ``rms_norm(residual) * norm_w`` (row-major, or
    fragment-packed with ``packed_out``).  GPU: gemm_skinny (packed ``wp``, split-K fp32 slabs)
    then reduce_add_rms_norm."""
    M, (N, K) = _rows(a, rows), skinny_wdims(wp)
    if splits is None:
        splits = 0  # automatic (launcher)
    if workspace is None:
        workspace = skinny_workspace(M, N, splits or skinny_auto_splits(M, N, K), a.device)
    s = skinny_slabs(a, wp, workspace, splits, rows=M)
    if out is None:
        out = (packed_empty(M, N, residual.dtype, a.device) if packed_out
               else torch.empty(M, N, dtype=residual.dtype, device=a.device))
    return reduce_add_rms_norm(out, residual, workspace, s, norm_w, eps)


def gemm_skinny(a: torch.Tensor, w: torch.Tensor, splits: int = 1) -> torch.Tensor:
    """``a @ w^T`` through the skinny kernel from a row-major weight (tests / tools)."""
    wp = pack_skinny(w)
    if splits == 1:
        return skinny_linear(a, wp)
    M, N = a.shape[0], w.shape[0]
    ws = skinny_workspace(M, N, splits, a.device)
    s = skinny_slabs(a, wp, ws, splits)
    return reduce_slabs(ws, s, M, N, a.dtype)


def layer_norm(x, w, b, eps):
    if not _gpu(x):
        return ref.layer_norm(x, w, b, eps)
    x = x.contiguous()
    out = torch.empty_like(x)
    native().layer_norm(out, x, w, b, eps)
    return out


def silu_mul(x: torch.Tensor, out: Optional[torch.Tensor] = None, interleaved: bool = False,
             pairing: Optional[int] = None) -> torch.Tensor:
    """silu(gate) * up over [.., 2F] gate_up activations: [F gate | F up], or ``interleaved``
    [64 gate | 64 up] per 128 columns (the output of the single resident, interleaved w13).
    ``pairing`` (where given, it decides): 0 and 1 name those two, 8 is [8 gate | 8 up] per 16
    columns - the output of a plain GEMM over a PACKED w13 (interleave_gate_up8)."""
    if pairing is None:
        pairing = 1 if interleaved else 0
    if pairing not in (0, 1, 8):
        raise ValueError(f"silu_mul: pairing {pairing!r} is not 0, 1 or 8")
    F2 = x.shape[-1]
    if pairing == 8 and F2 % 16:
        raise ValueError(f"silu_mul: {F2} gate_up columns are no whole [8 gate | 8 up] groups")
    if not _gpu(x):
        y = ref.silu_mul(x, pairing=pairing)
        return out.copy_(y) if out is not None else y
    if out is None:
        out = torch.empty(*x.shape[:-1], F2 // 2, dtype=x.dtype, device=x.device)
    native().silu_mul_pairing(out, x.contiguous(), pairing)
    return out


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    if not _gpu(x):
        return ref.gelu_tanh(x)
    x = x.contiguous()
    out = torch.empty_like(x)
    native().gelu_tanh(out, x)
    return out


def embedding(ids: torch.Tensor, weight: torch.Tensor, vocab_start: int = 0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if not _gpu(weight):
        return ref.embedding(ids, weight, vocab_start)
    if out is None:
        out = torch.empty(ids.numel(), weight.shape[1], dtype=weight.dtype, device=weight.device)
    native().embedding(out, ids, weight, vocab_start)
    return out


def embed_norm_partial(ids: torch.Tensor, weight: torch.Tensor, norm_w: torch.Tensor,
                       src: Optional[torch.Tensor] = None, prev: Optional[torch.Tensor] = None,
                       packed: bool = True) -> tuple:
    """The decode step's front end: the (pipelined, see :func:`resolve_ids`) input ids' embedding
    rows and the first layer's deferred-norm operands - ``(residual [M, d], residual * norm_w
    (fragment-packed), ss_part [M, d/512])``, what embedding + add_norm_partial(nslabs=0) return,
    in one launch."""
    M, d = ids.numel(), weight.shape[1]
    if not _gpu(weight):
        if src is not None:
            ids = resolve_ids(ids, src, prev)
        res = ref.embedding(ids, weight, 0).contiguous()
        xw, ss = add_norm_partial(res, None, 0, norm_w, packed=packed)
        return res, xw, ss
    res = torch.empty(M, d, dtype=weight.dtype, device=weight.device)
    ss = torch.empty(M, d // 512, dtype=torch.float32, device=weight.device)
    out = packed_empty(M, d, weight.dtype, weight.device) if packed else torch.empty_like(res)
    native().embed_norm_partial(out, res, ids, src, prev, weight, norm_w, ss)
    return res, out, ss


def resolve_ids(ids: torch.Tensor, src: torch.Tensor, prev: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode input ids under pipelining: ``prev[src[i]]`` where ``src[i] >= 0`` (the token the
    previous step sampled in that row, still on the device), else ``ids[i]``."""
    if not _gpu(ids):
        return torch.where(src >= 0, prev.index_select(0, src.clamp(min=0).long()), ids)
    if out is None:
        out = torch.empty_like(ids)
    native().resolve_ids(out, ids, src, prev)
    return out


# ---------------------------------------------------------------- attention

def rope_and_cache(qkv: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor,
                   k_cache: Optional[torch.Tensor], v_cache: Optional[torch.Tensor],
                   slot_mapping: Optional[torch.Tensor], Hq: int, Hkv: int, D: int,
                   apply_rope: bool = True, partial: Optional[torch.Tensor] = None, nslabs: int = 0,
                   kv_scale: Optional[torch.Tensor] = None, qk_norm: Optional[tuple] = None) -> None:
    """In place: rotate q and k inside the fused QKV rows; write k, v into the paged cache.
    With ``partial`` (GPU), the QKV values are first reduced from ``nslabs`` fp32 split-K slabs
    [nslabs, T, (Hq+2Hkv)*D] (skinny_slabs) and the reduced rows are written to ``qkv``.
    An e4m3 cache (``kv_scale`` its scales, :func:`kv_cache_alloc`) takes every token quantised
    from the rotated rows (:func:`quantize_kv`).
    ``qk_norm = (q_w, k_w, eps)`` (Qwen3): every q head and every k head is RMS-normalised over
    its D values and scaled by ``q_w`` / ``k_w`` ([D], fp32 or bf16) before the rotation, in fp32
    inside the same kernel - the rows and the K cache still see one rounding to bf16."""
    qw = kw = None
    eps = 0.0
    if qk_norm is not None:
        qw, kw, eps = qk_norm
        for w in (qw, kw):
            if not isinstance(w, torch.Tensor) or w.shape != (D,):
                raise ValueError(f"qk_norm weights must be [D = {D}] tensors")
            if w.device != qkv.device or w.dtype != qw.dtype or w.dtype not in (torch.float32, torch.bfloat16):
                raise ValueError("qk_norm weights must be on qkv's device, both fp32 or both bf16")
        eps = float(eps)
    if not _gpu(qkv):
        if partial is not None:
            T, n = qkv.shape[0], qkv.shape[1]
            qkv.copy_(partial[: nslabs * T * n].view(nslabs, T, n).sum(0).to(qkv.dtype))
        ref.rope_and_cache(qkv, positions, cos_sin, k_cache, v_cache, slot_mapping, Hq, Hkv, D, apply_rope,
                           kv_scale=kv_scale, qk_norm=qk_norm)
        return
    empty = _empty_i32(qkv.device)
    native().rope_and_cache(qkv, positions, cos_sin,
                            k_cache if k_cache is not None else empty,
                            v_cache if v_cache is not None else empty,
                            slot_mapping if slot_mapping is not None else empty,
                            Hq, Hkv, D, apply_rope, partial, nslabs,
                            kv_scale if k_cache is not None and slot_mapping is not None else None,
                            qw, kw, eps)


_EMPTY = {}


def _empty_i32(device) -> torch.Tensor:
    t = _EMPTY.get(device)
    if t is None:
        t = _EMPTY[device] = torch.empty(0, dtype=torch.int32, device=device)
    return t


MAX_SPLITS = 64  # kPdMaxSplits

# The compiled forms of paged decode attention as (head dim, query heads per KV head, fused, fp8
# cache): the rows of kPdForms in csrc/paged_decode_forms.h, which native().paged_decode_forms()
# reports (tests/test_attn_decode_plan_cpu.py compares the two).  Each row is compiled for both
# chunk widths, a fused row also with and without the in-launch merge.  Kept here as well because
# the model and the engine choose their decode path by it with no extension built.
PD_FORMS: tuple = (
    tuple((128, g, 0, 0) for g in (1, 2, 4, 8, 16)) + tuple((64, g, 0, 0) for g in (1, 2, 4, 8))
    + tuple((128, g, 0, 1) for g in (1, 2, 4, 8, 16))
    + tuple((128, g, 1, f8) for f8 in (0, 1) for g in (1, 2, 4, 8)))  # fused: no G = 16
_PD_GS: dict = {}  # the table by key (every decode layer's setup asks it): (D, fused, f8) -> the row's Gs
for _f in PD_FORMS:
    _PD_GS.setdefault((_f[0], _f[2], _f[3]), set()).add(_f[1])


def paged_decode_why(D: int, G: Optional[int], fused: bool = False, f8: bool = False) -> Optional[str]:
    """THE rule of paged decode's forms, pd_plan's twin (csrc/paged_decode_forms.h;
    tests/test_attn_decode_plan_cpu.py sweeps the two against each other): None where PD_FORMS has
    a form for head dim ``D`` with ``G`` query heads per KV head (None: with any), ``fused``
    (paged_decode_fused) or not, over an e4m3 cache (``f8``) or a bf16 one; else the reason.  Asked
    for the GPU only: the CPU reference takes any shape."""
    gs = _PD_GS.get((D, int(fused), int(f8)))
    if gs is not None and (G is None or G in gs):
        return None
    what = f"{'fused ' if fused else ''}paged decode{' over an fp8 KV cache' if f8 else ''}"
    if (f8 or fused) and D != 128:
        return f"{what} needs head_dim 128 on the GPU, not {D}"
    if gs is None:
        return f"{what}: no form for head_dim {D}"
    return f"{what}: head_dim {D} has forms for {sorted(gs)} query heads per KV head, not {G}"


def decode_splits(batch: int, Hkv: int, n_cu: int = 256) -> int:
    """Splits per (sequence, kv head) for paged_decode: aim for ~one workgroup per CU in total.

    Measured on MI355X (tools/bench_decode.py, ctx 1.8k-6k): batch 64 x 8 kv heads is best
    unsplit (83 us, 5.7 TB/s - a merge launch and extra partial traffic only cost), batch 8 at 4
    splits, batch 1 at 16-32 splits."""
    return max(1, min(32, round(n_cu / max(1, batch * Hkv))))


# split partials of paged_decode_fused merged inside the attention launch by the last-arriving
# split (no paged_decode_reduce launch); the decode workspace carries the hand-off counters
DECODE_MERGE = True


def decode_workspace(max_batch: int, Hq: int, D: int, max_model_len: int = 0, device=None, Hkv: Optional[int] = None):
    """fp32 partials of the split-K decode kernel: [B, Hq, MAX_SPLITS, D] and [.., 2], plus the
    in-launch merge's (sequence, kv head) counters (int32, zero; each launch leaves them zero)."""
    part_out = torch.empty(max_batch, Hq, MAX_SPLITS, D, dtype=torch.float32, device=device)
    part_ml = torch.empty(max_batch, Hq, MAX_SPLITS, 2, dtype=torch.float32, device=device)
    ctr = torch.zeros(max_batch * Hq, dtype=torch.int32, device=device)
    return part_out, part_ml, ctr


def paged_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                 seq_lens: torch.Tensor, Hq: int, Hkv: int, D: int, scale: float,
                 workspace: Optional[tuple] = None, out: Optional[torch.Tensor] = None,
                 splits: Optional[int] = None, kv_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    if not _gpu(q):
        r = cpu_attn.paged_decode(q, k_cache, v_cache, block_tables, seq_lens, Hq, Hkv, D, scale, kv_scale=kv_scale)
        if out is not None and out.dim() == 4:  # fragment-packed output (gemm_skinny A operand)
            r = pack_activation(r)
        return out.copy_(r) if out is not None else r
    B = seq_lens.shape[0]
    if workspace is None:
        workspace = decode_workspace(B, Hq, D, device=q.device)
    if out is None:
        out = torch.empty(B, Hq * D, dtype=q.dtype, device=q.device)
    S = splits or decode_splits(B, Hkv)
    native().paged_decode(out, q, k_cache, v_cache, block_tables, seq_lens, workspace[0], workspace[1],
                          Hq, Hkv, D, scale, S, kv_scale)
    return out


def paged_decode_fused(slabs: torch.Tensor, nslabs: int, positions: torch.Tensor, cos_sin: torch.Tensor,
                       slot_mapping: Optional[torch.Tensor], k_cache: torch.Tensor, v_cache: torch.Tensor,
                       block_tables: torch.Tensor, seq_lens: torch.Tensor, Hq: int, Hkv: int, D: int, scale: float,
                       workspace: Optional[tuple] = None, out: Optional[torch.Tensor] = None,
                       splits: Optional[int] = None, kv_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """paged_decode with rope_and_cache folded in: the new token's q / k / v are the sum of the qkv
    projection's ``nslabs`` fp32 split-K slabs [nslabs, B, (Hq + 2 Hkv) * D] (skinny_slabs),
    rounded to the cache dtype, q / k rotated at ``positions``, k / v written to the cache at
    ``slot_mapping``; attention over the cached tokens plus the new one (D = 128 on the GPU).
    With an e4m3 cache (``kv_scale``) the new token is quantised in the kernel and attended
    dequantised, as every later step will read it."""
    B = seq_lens.shape[0]
    act = torch.bfloat16 if is_fp8(k_cache) else k_cache.dtype
    if not _gpu(slabs):
        n = (Hq + 2 * Hkv) * D
        qkv = slabs[: nslabs * B * n].view(nslabs, B, n).sum(0).to(act)
        ref.rope_and_cache(qkv, positions, cos_sin, k_cache, v_cache, slot_mapping, Hq, Hkv, D, True,
                           kv_scale=kv_scale)
        return paged_decode(qkv, k_cache, v_cache, block_tables, seq_lens, Hq, Hkv, D, scale, out=out,
                            kv_scale=kv_scale)
    if workspace is None:
        workspace = decode_workspace(B, Hq, D, device=slabs.device)
    if out is None:
        out = torch.empty(B, Hq * D, dtype=act, device=slabs.device)
    S = splits or decode_splits(B, Hkv)
    merge = workspace[2] if DECODE_MERGE and len(workspace) > 2 else _empty_i32(slabs.device)
    native().paged_decode_fused(out, slabs, nslabs, positions, cos_sin,
                                slot_mapping if slot_mapping is not None else _empty_i32(slabs.device),
                                k_cache, v_cache, block_tables, seq_lens, workspace[0], workspace[1], Hq, Hkv, D,
                                scale, S, merge, kv_scale)
    return out


def prefill_qblocks(cu_seqlens_cpu: list[int], block: int = 128, ctx_starts: Optional[list[int]] = None,
                    order: str = "seq") -> tuple[list[int], list[int]]:
    """Q-block schedule for flash_prefill: (seq index, first q row) per 128-row block.  A block's
    work is its causal key span: the sequence's cached prefix (``ctx_starts``, chunked prefill)
    plus its first row.

    ``order="seq"`` (the engine's, sequence-major): the longest sequence first, each sequence's
    blocks heaviest first.  The workgroups resident on one XCD at a time (one kv head's) then cover
    one or two sequences, whose K/V stay in that XCD's 4 MiB L2, and the grid still ends on light
    blocks: 10 x 1609 tokens 276.7 vs 295.1 us, 64 x 1609 1788 vs 1934 us
    (profiles/r04/flash_qb_order_nw.jsonl).  ``work``: all blocks heaviest first across sequences,
    so the residents span ~10 sequences' K/V."""
    items = []
    for i in range(len(cu_seqlens_cpu) - 1):
        n = cu_seqlens_cpu[i + 1] - cu_seqlens_cpu[i]
        c = ctx_starts[i] if ctx_starts is not None else 0
        for s in range(0, n, block):
            items.append((c + s, s, i, c + n))
    if order == "seq":
        items.sort(key=lambda t: (-t[3], t[2], -t[0]))
    else:
        items.sort(key=lambda t: -t[0])
    return [t[2] for t in items], [t[1] for t in items]


def flash_prefill(qkv: torch.Tensor, cu_seqlens: torch.Tensor, Hq: int, Hkv: int, D: int, scale: float,
                  qblocks: Optional[tuple[torch.Tensor, torch.Tensor]] = None,
                  out: Optional[torch.Tensor] = None, paged: Optional[tuple] = None,
                  kv_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal varlen attention of the prefill rows.  ``paged = (ctx_start, k_cache, v_cache,
    block_tables)``: each sequence's rows are its NEW tokens at positions ctx_start.. and the
    keys/values (cached prefix + new) are read from the paged cache.  With an e4m3 cache
    (``kv_scale``) only the cached prefix is read from the cache (dequantised); this step's own
    tokens are attended unquantised from the qkv rows (the v1 kernel's fp8 form)."""
    if not _gpu(qkv):
        if paged is not None:
            cs, kc, vc, bt = paged
            return cpu_attn.paged_prefill(qkv, cu_seqlens, cs, kc, vc, bt, Hq, Hkv, D, scale, kv_scale=kv_scale)
        return cpu_attn.flash_prefill(qkv, cu_seqlens, Hq, Hkv, D, scale)
    if qblocks is None:
        qs, st = prefill_qblocks(cu_seqlens.tolist())
        qblocks = (torch.tensor(qs, dtype=torch.int32, device=qkv.device),
                   torch.tensor(st, dtype=torch.int32, device=qkv.device))
    if out is None:
        out = torch.empty(qkv.shape[0], Hq * D, dtype=qkv.dtype, device=qkv.device)
    if paged is not None:
        cs, kc, vc, bt = paged
        native().flash_prefill(out, qkv, cu_seqlens, qblocks[0], qblocks[1], Hq, Hkv, D, scale, cs, kc, vc, bt,
                               kv_scale)
    else:
        native().flash_prefill(out, qkv, cu_seqlens, qblocks[0], qblocks[1], Hq, Hkv, D, scale, None, None, None,
                               None, None)
    return out


# ---------------------------------------------------------------- sampling

class PenaltyState:
    """Per-sequence token counts for the sampling penalties (``ref.apply_penalties``), resident
    on the sampler's device so a captured decode step reads and updates them itself.

    ``table`` int16 ``[slots, stride]`` (stride = V rounded up to 8, so every row is 16-byte
    aligned): bit 15 = the token is in the prompt, bits 0..14 = how often it was generated,
    saturating at ``MAX_COUNT``.  ``params`` fp32 ``[slots, 4]``: (rep, fp32(1 / rep), presence,
    frequency) per slot.  A sampler row names its slot through ``ops.sample(..., slots=)``."""

    MAX_COUNT = 0x7FFF
    SEEN = -0x8000  # bit 15 of an int16

    def __init__(self, slots: int, V: int, device):
        self.slots, self.V = int(slots), int(V)
        self.device = torch.device(device)
        stride = (self.V + 7) // 8 * 8
        self.table = torch.zeros(self.slots, stride, dtype=torch.int16, device=self.device)
        self.params = torch.tensor([[1.0, 1.0, 0.0, 0.0]] * self.slots, dtype=torch.float32, device=self.device)
        self.device = self.table.device  # with its index ("cuda" -> "cuda:0")

    @property
    def nbytes(self) -> int:
        return self.table.numel() * 2 + self.params.numel() * 4

    def reset(self, slot: int, prompt_ids, output_ids, rep: float = 1.0, presence: float = 0.0,
              frequency: float = 0.0) -> None:
        """Make ``slot`` describe one sequence: clear its row, mark ``prompt_ids`` as seen, count
        ``output_ids`` and set its parameters.  Enqueued on the current stream; no host sync."""
        if not 0 <= slot < self.slots:
            raise ValueError(f"slot {slot} outside [0, {self.slots})")
        if not rep > 0:
            raise ValueError("repetition penalty must be > 0")
        inv = ref.penalty_inv_rep(rep)
        n_p, n_o = len(prompt_ids), len(output_ids)
        ids = torch.tensor(list(prompt_ids) + list(output_ids), dtype=torch.int32)
        if self.device.type == "cuda":
            ids = ids.pin_memory().to(self.device, non_blocking=True)
            native().penalty_reset(self.table, self.params, self.V, slot, ids, n_p, n_o, rep, inv, presence,
                                   frequency)
            return
        row = self.table[slot]
        row.zero_()
        ids = ids.long()
        ok = (ids >= 0) & (ids < self.V)
        row[ids[:n_p][ok[:n_p]]] = self.SEEN
        cnt = torch.bincount(ids[n_p:][ok[n_p:]], minlength=self.V).clamp_(max=self.MAX_COUNT)
        row[: self.V] |= cnt.to(torch.int16)
        self.params[slot] = torch.tensor([rep, inv, presence, frequency], dtype=torch.float32)

    def counts(self) -> torch.Tensor:
        """int32 ``[slots, V]``: how often each token was generated."""
        return (self.table[:, : self.V].to(torch.int32) & self.MAX_COUNT)

    def seen(self) -> torch.Tensor:
        """bool ``[slots, V]``: the token is in the slot's prompt."""
        return self.table[:, : self.V] < 0


class GuideState:
    """Constrained decoding on the sampler's device (engine/guide.py compiles the guides): an
    arena of DFA states, one row each, and the guide state of every sequence slot, so a captured
    decode step masks its logits and advances its guides by itself.

    * the vocabulary as CSR: ``tok_off`` int32 ``[V + 1]`` and ``blob`` uint8;
    * ``mask`` ``[rows, W]`` 32-bit words (stored as int32), ``W = ceil(V / 32)`` rounded up to 4
      words so every row is 16-byte aligned: token ``t`` is bit ``t & 31`` of word ``t >> 5``
      (``ref.guide_mask``); ``popc`` int32 ``[rows]`` counts a row's allowed tokens;
    * ``trans`` int32 ``[rows, 256]`` holding **absolute** row numbers (-1 dead), ``accept`` uint8
      ``[rows]``;
    * ``state`` int32 ``[slots]``: the slot's current absolute row, -1 = unguided.

    Rows are handed out one by one from ``free_rows``; transitions are absolute, so a guide's rows
    need not be contiguous and the arena cannot fragment.  Resident guides are keyed by their
    canonical spec text, ref-counted by the slots using them and evicted least recently used, when
    unreferenced, once rows run out.  A sampler row names its slot through
    ``ops.sample(..., guide=, gslots=)``."""

    def __init__(self, slots: int, V: int, vocab_bytes, eos_ids, device, rows: int):
        import numpy as np

        self.slots, self.V, self.rows = int(slots), int(V), int(rows)
        if len(vocab_bytes) != self.V:
            raise ValueError(f"vocab_bytes has {len(vocab_bytes)} entries, the vocabulary {self.V}")
        if self.slots <= 0 or self.rows <= 0:
            raise ValueError("a guide state needs slots and rows")
        self.vocab_bytes = [bytes(b) for b in vocab_bytes]
        self.eos_ids = tuple(sorted({int(t) for t in eos_ids}))
        self.W = ((self.V + 31) // 32 + 3) // 4 * 4
        dev = torch.device(device)
        off = np.zeros(self.V + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(b) for b in self.vocab_bytes])
        if off[-1] >= 1 << 31:
            raise ValueError("vocabulary bytes exceed 2 GiB")
        blob = np.frombuffer(b"".join(self.vocab_bytes) + b"\0", dtype=np.uint8).copy()  # never empty
        self.tok_off = torch.from_numpy(off.astype(np.int32)).to(dev)
        self.blob = torch.from_numpy(blob).to(dev)
        self.eos = torch.tensor(self.eos_ids, dtype=torch.int32, device=dev)
        self.mask = torch.zeros(self.rows, self.W, dtype=torch.int32, device=dev)
        self.popc = torch.zeros(self.rows, dtype=torch.int32, device=dev)
        self.trans = torch.full((self.rows, 256), -1, dtype=torch.int32, device=dev)
        self.accept = torch.zeros(self.rows, dtype=torch.uint8, device=dev)
        self.state = torch.full((self.slots,), -1, dtype=torch.int32, device=dev)
        self.device = self.mask.device  # with its index ("cuda" -> "cuda:0")
        self.free_rows: list = list(range(self.rows - 1, -1, -1))
        self._resident: "OrderedDict[str, list]" = OrderedDict()  # key -> [guide, rows (np), refs]
        self._slot_key: dict = {}
        # with every single-byte token in the vocabulary no reachable state can have an empty row
        self._all_bytes = len({b for b in self.vocab_bytes if len(b) == 1}) == 256

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.tok_off, self.blob, self.eos, self.mask, self.popc,
                                                          self.trans, self.accept, self.state))

    @property
    def guides_resident(self) -> int:
        return len(self._resident)

    @property
    def slots_in_use(self) -> int:
        return len(self._slot_key)

    def resident_rows(self, guide):
        """The absolute rows of a resident guide (state i in ``rows[i]``), or None."""
        r = self._resident.get(guide.key)
        return None if r is None else r[1]

    def load(self, guide):
        """Make ``guide`` resident (upload ``trans`` / ``accept``, build its mask rows on the
        current stream) and return its absolute rows.  ``ValueError`` for a guide with a
        non-accepting state whose row is empty (a vocabulary lacking some single-byte token);
        ``RuntimeError`` when its rows cannot be found even after evicting every unreferenced guide."""
        import numpy as np

        r = self._resident.get(guide.key)
        if r is not None:
            self._resident.move_to_end(guide.key)
            return r[1]
        n = guide.n
        while len(self.free_rows) < n:
            victim = next((k for k, v in self._resident.items() if v[2] == 0), None)
            if victim is None:
                raise RuntimeError(f"guide arena full: {n} rows needed, {len(self.free_rows)} free of {self.rows}")
            self.free_rows.extend(int(x) for x in self._resident.pop(victim)[1][::-1])
        rows = np.array([self.free_rows.pop() for _ in range(n)], dtype=np.int64)
        t = np.asarray(guide.trans)
        t_abs = np.where(t >= 0, rows[np.maximum(t, 0)], -1).astype(np.int32)
        acc = np.asarray(guide.accept).astype(np.uint8)
        rows_t = torch.from_numpy(rows)
        if self.device.type == "cuda":
            rows_d = rows_t.to(torch.int32).pin_memory().to(self.device, non_blocking=True)
            idx = rows_d.long()
            self.trans[idx] = torch.from_numpy(t_abs).pin_memory().to(self.device, non_blocking=True)
            self.accept[idx] = torch.from_numpy(acc).pin_memory().to(self.device, non_blocking=True)
            native().guide_mask_build(self.mask, self.trans, self.accept, self.popc, rows_d, self.tok_off, self.blob,
                                      self.eos)
        else:
            ok = ref.guide_mask(t, guide.accept, self.vocab_bytes, self.eos_ids).numpy()
            bits = np.zeros((n, self.W * 32), dtype=bool)
            bits[:, : self.V] = ok
            words = np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)
            self.trans[rows_t] = torch.from_numpy(t_abs)
            self.accept[rows_t] = torch.from_numpy(acc)
            self.mask[rows_t] = torch.from_numpy(words.copy())
            self.popc[rows_t] = torch.from_numpy(ok.sum(1).astype(np.int32))
        if not self._all_bytes:  # the only case with a possibly empty row: worth one readback
            empty = (self.popc[rows_t.to(self.device)].cpu().numpy() == 0) & (acc == 0)
            if empty.any():
                self.free_rows.extend(int(x) for x in rows[::-1])
                raise ValueError(f"guide state {int(np.flatnonzero(empty)[0])} allows no token of this vocabulary "
                                 "(it lacks some single-byte token)")
        self._resident[guide.key] = [guide, rows, 0]
        return rows

    def walk(self, guide, output_token_ids) -> int:
        """The guide's own state after the given tokens, by the sampler's rules: an eos token, a
        token outside ``[0, V)``, a token without bytes and a walk that would die leave it."""
        s = 0
        for t in output_token_ids:
            t = int(t)
            if not 0 <= t < self.V or t in self.eos_ids or not self.vocab_bytes[t]:
                continue
            nxt = ref.guide_advance(guide.trans, s, self.vocab_bytes[t])
            if nxt >= 0:
                s = nxt
        return s

    def reset(self, slot: int, guide, output_token_ids=()) -> None:
        """Make ``slot`` follow ``guide`` from its start state advanced over ``output_token_ids``
        (walked on the host); the slot's state is written on the current stream, no host sync."""
        if not 0 <= slot < self.slots:
            raise ValueError(f"slot {slot} outside [0, {self.slots})")
        rows = self.load(guide)
        self._drop(slot)
        self._resident[guide.key][2] += 1
        self._slot_key[slot] = guide.key
        self.state[slot:slot + 1].fill_(int(rows[self.walk(guide, output_token_ids)]))

    def _drop(self, slot: int) -> None:
        key = self._slot_key.pop(slot, None)
        if key is not None:
            self._resident[key][2] -= 1

    def release(self, slot: int) -> None:
        """The slot follows no guide any more (stream-ordered like :meth:`reset`)."""
        self._drop(slot)
        self.state[slot:slot + 1].fill_(-1)

    def mask_bits(self, rows) -> torch.Tensor:
        """bool ``[len(rows), V]`` (host): the mask rows unpacked."""
        import numpy as np

        idx = torch.as_tensor(np.asarray(rows, dtype=np.int64)).to(self.device)
        w = self.mask[idx].cpu().numpy().view(np.uint32).astype("<u4")
        return torch.from_numpy(np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, : self.V].astype(bool))


def sample(logits: torch.Tensor, temperature: Optional[torch.Tensor] = None, top_k: Optional[torch.Tensor] = None,
           top_p: Optional[torch.Tensor] = None, rng: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, advance: bool = False, penalties: Optional[PenaltyState] = None,
           slots: Optional[torch.Tensor] = None, guide: Optional[GuideState] = None,
           gslots: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Next tokens [B] int32.  temperature <= 0 (or None) is greedy.  ``advance``: bump the RNG
    counter ``rng[1]`` after drawing (on the GPU inside the final sampling kernel - no extra
    launch inside a captured decode step).  ``penalties`` with ``slots`` (int32 [B], -1 = none):
    row b's logits are penalised by the state's slot ``slots[b]`` first (``ref.apply_penalties``),
    and the token drawn is counted there (distinct rows must name distinct slots).  ``guide`` with
    ``gslots`` (int32 [B], -1 = none): a row whose slot holds a state reads its (penalised) logits
    through that state's token mask - disallowed tokens are -inf - and the token drawn advances the
    slot's state (distinct rows must name distinct slots)."""
    if guide is not None:
        if gslots is None or gslots.dtype != torch.int32 or gslots.numel() < logits.shape[0]:
            raise ValueError("a guide needs gslots: int32 [B]")
        if guide.V != logits.shape[1] or guide.device != logits.device:
            raise ValueError("the guide state belongs to another vocabulary or device")
    if penalties is not None:
        if slots is None or slots.dtype != torch.int32 or slots.numel() < logits.shape[0]:
            raise ValueError("penalties need slots: int32 [B]")
        if penalties.V != logits.shape[1] or penalties.device != logits.device:
            raise ValueError("the penalty state belongs to another vocabulary or device")
    if not _gpu(logits):
        r = _sample_cpu(logits, temperature, top_k, top_p, rng, penalties, slots, guide, gslots)
        if advance and rng is not None:
            rng[1] += 1
        return out.copy_(r) if out is not None else r
    if out is None:
        out = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    pen = () if penalties is None else (penalties.table, penalties.params, slots, penalties.V)
    if guide is not None:
        pen = pen or (None, None, None, 0)
        pen += (guide.mask, guide.trans, guide.state, gslots, guide.tok_off, guide.blob, guide.eos)
    native().sample(out, logits, temperature, top_k, top_p, rng, advance and rng is not None, *pen)
    return out


def _sample_cpu(logits, temperature, top_k, top_p, rng, penalties=None, slots=None, guide=None, gslots=None):
    B = logits.shape[0]
    res = torch.empty(B, dtype=torch.int32)
    gen = torch.Generator().manual_seed(int(rng[0]) * 1000003 + int(rng[1])) if rng is not None else None
    for b in range(B):
        t = float(temperature[b]) if temperature is not None else 0.0
        row = logits[b]
        slot = int(slots[b]) if penalties is not None else -1
        if penalties is not None and slot >= penalties.slots:
            slot = -1  # like the kernel: a slot the state does not have is no slot
        if slot >= 0:
            rep, _, pres, freq = penalties.params[slot].tolist()
            e = penalties.table[slot, : penalties.V]
            row = ref.apply_penalties(row, e < 0, e.to(torch.int32) & PenaltyState.MAX_COUNT, rep, pres, freq)
        gs = int(gslots[b]) if guide is not None else -1
        st = int(guide.state[gs]) if 0 <= gs < (guide.slots if guide is not None else 0) else -1
        if not 0 <= st < (guide.rows if guide is not None else 0):
            st = -1  # like the kernel: no slot, or a slot without a state, is no guide
        if st >= 0:
            row = row.float().masked_fill(~guide.mask_bits([st])[0], float("-inf"))
        x = row.float()
        if t <= 0:
            res[b] = int(x.argmax())
        else:
            keep = ref.sample_keep(row, t, int(top_k[b]) if top_k is not None else 0,
                                   float(top_p[b]) if top_p is not None else 1.0)
            x = (x / t).masked_fill(~keep, float("-inf"))
            res[b] = int(torch.multinomial(torch.softmax(x, -1), 1, generator=gen))
        if slot >= 0:  # count the drawn token, saturating
            e = penalties.table[slot, int(res[b])]
            if int(e) & PenaltyState.MAX_COUNT != PenaltyState.MAX_COUNT:
                penalties.table[slot, int(res[b])] = e + 1
        tok = int(res[b])
        if st >= 0 and 0 <= tok < guide.V and tok not in guide.eos_ids and guide.vocab_bytes[tok]:
            nxt = ref.guide_advance(guide.trans, st, guide.vocab_bytes[tok])  # absolute rows
            if 0 <= nxt < guide.rows:
                guide.state[gs] = nxt
    return res


# ---------------------------------------------------------------- token log-probabilities

LP_MAX_TOP = 20  # kLpMaxTop: OpenAI's top_logprobs limit
LP_WIDTH = 1 + 2 * LP_MAX_TOP  # int32 words of one row's packed record


def token_logprobs(logits: torch.Tensor, tokens: torch.Tensor, want: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Log-probabilities of the drawn tokens and of the most likely alternatives
    (``ref.token_logprobs``): the model's distribution over the logits as given, before penalties,
    temperature and top-k / top-p.  ``tokens`` int32 [B] (what ``sample`` wrote), ``want`` int32
    [B]: < 0 the row did not ask (its record is left as it is), 0 the token's logprob only,
    1..``LP_MAX_TOP`` plus that many alternatives.  Returns ``out``: int32 ``[B, LP_WIDTH]``, per
    row word 0 = the bits of lp(token), words 1..20 = the bits of the alternatives' logprobs,
    words 21..40 = their ids (``unpack_logprobs``) - one buffer, so a step's logprobs reach the
    host in one copy."""
    B = logits.shape[0]
    if tokens.dtype != torch.int32 or want.dtype != torch.int32 or tokens.numel() < B or want.numel() < B:
        raise ValueError("token_logprobs: tokens and want are int32 [B]")
    if out is None:
        out = torch.zeros(B, LP_WIDTH, dtype=torch.int32, device=logits.device)
    elif out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] < B or out.shape[1] != LP_WIDTH:
        raise ValueError(f"token_logprobs: out is int32 [>= B, {LP_WIDTH}]")
    if _gpu(logits):
        native().token_logprobs(out, logits, tokens, want)
        return out
    for b in range(B):
        n = min(int(want[b]), LP_MAX_TOP)
        if n < 0:
            continue
        lp, ids, lps = ref.token_logprobs(logits[b], int(tokens[b]), n)
        rec = out[b]
        rec[0] = torch.tensor(lp, dtype=torch.float32).view(torch.int32)
        rec[1:1 + LP_MAX_TOP] = torch.tensor(float("-inf"), dtype=torch.float32).view(torch.int32)
        rec[1 + LP_MAX_TOP:] = -1
        rec[1:1 + n] = lps.view(torch.int32)
        rec[1 + LP_MAX_TOP:1 + LP_MAX_TOP + n] = ids
    return out


def pool_l2(x: torch.Tensor, dim, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Last-token pooling of embedding requests (``ref.pool_l2``): row ``r`` of ``x`` (bf16 or
    fp32 [R, d], the final-normed hidden rows; a view with a wider row stride is fine) cut to its
    first ``dim[r]`` columns and L2-normalised into ``out`` fp32 [R, d], zeros beyond them.  Rows
    with ``dim[r] <= 0`` are left as they are in ``out`` (zeros in a fresh one).  ``dim`` is int32
    [R] on ``x``'s device, or host values (a list or a CPU tensor), which are checked against ``d``
    here; values already on the GPU are not read back, the kernel clamps them to ``d``."""
    if x.dim() != 2 or x.dtype not in (torch.bfloat16, torch.float32) or (x.shape[1] and x.stride(1) != 1):
        raise ValueError(f"pool_l2: x is bf16 or fp32 [R, d] with unit column stride, got {x.dtype} {list(x.shape)}")
    R, d = x.shape
    if not isinstance(dim, torch.Tensor) or not dim.is_cuda:
        dim = torch.as_tensor(dim).reshape(-1)
        if dim.is_floating_point() or dim.numel() < R:
            raise ValueError("pool_l2: dim holds R integers")
        if R and int(dim[:R].max()) > d:
            raise ValueError(f"pool_l2: dim {int(dim[:R].max())} exceeds the row width {d}")
        dim = dim.to(device=x.device, dtype=torch.int32)
    elif dim.dtype != torch.int32 or dim.numel() < R or dim.device != x.device:
        raise ValueError("pool_l2: dim is int32 [R] on x's device")
    if out is None:
        out = torch.zeros(R, d, dtype=torch.float32, device=x.device)
    elif (out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (R, d) or not out.is_contiguous()
          or out.device != x.device):
        raise ValueError(f"pool_l2: out is contiguous fp32 [{R}, {d}] on x's device")
    if not _gpu(x):
        return ref.pool_l2(x, dim, out)
    if R and d:
        native().pool_l2(out, x, dim.contiguous())
    return out


def unpack_logprobs(rec_row) -> tuple:
    """``(lp, [(id, lp), ...])`` of one packed record (a host int32 row of ``token_logprobs``):
    the alternatives up to the first empty entry."""
    rec = torch.as_tensor(rec_row, dtype=torch.int32).contiguous()
    f = rec.view(torch.float32).tolist()
    ids = rec[1 + LP_MAX_TOP:].tolist()
    top = []
    for j, i in enumerate(ids):
        if i < 0:
            break
        top.append((i, f[1 + j]))
    return f[0], top


# ---------------------------------------------------------------- mixture of experts

def moe_route(router_logits: torch.Tensor, k: int, renorm: bool = True):
    if not _gpu(router_logits):
        return ref.moe_route(router_logits, k, renorm)
    T = router_logits.shape[0]
    lf = router_logits.float().contiguous()
    ids = torch.empty(T, k, dtype=torch.int32, device=lf.device)
    w = torch.empty(T, k, dtype=torch.float32, device=lf.device)
    native().moe_route(lf, ids, w, renorm)
    return ids, w


def moe_router(x: torch.Tensor, router_w: torch.Tensor, k: int, renorm: bool = True) -> tuple:
    """MoE decode routing in one launch: ``(ids [T, k] int32, w [T, k] fp32, wd [T, E] fp32)`` -
    the top-k experts of bf16(x . router_w^T), their (renormalised) softmax weights, and the dense
    per-expert weight rows (0 where an expert was not chosen) for the grouped expert kernels."""
    T, E = x.shape[0], router_w.shape[0]
    if not _gpu(x) or E > 16:
        ids, w = moe_route(torch.nn.functional.linear(x, router_w).float(), k, renorm)
        wd = torch.zeros(T, E, dtype=torch.float32, device=x.device).scatter_(1, ids.long(), w)
        return ids, w, wd
    ids = torch.empty(T, k, dtype=torch.int32, device=x.device)
    w = torch.empty(T, k, dtype=torch.float32, device=x.device)
    wd = torch.empty(T, E, dtype=torch.float32, device=x.device)
    native().moe_router(x.contiguous(), router_w, ids, w, wd, renorm)
    return ids, w, wd


def moe_align(ids: torch.Tensor, E: int):
    if not _gpu(ids) or E > 16:
        return ref.moe_align(ids, E)
    n = ids.numel()
    offsets = torch.empty(E + 1, dtype=torch.int32, device=ids.device)
    sorted_idx = torch.empty(n, dtype=torch.int32, device=ids.device)
    inv_idx = torch.empty(n, dtype=torch.int32, device=ids.device)
    native().moe_align(ids.contiguous(), E, offsets, sorted_idx, inv_idx)
    return offsets, sorted_idx, inv_idx


def gather_rows(x: torch.Tensor, idx: torch.Tensor, div: int = 1) -> torch.Tensor:
    if not _gpu(x):
        return x[(idx.long() // div)]
    out = torch.empty(idx.numel(), x.shape[1], dtype=x.dtype, device=x.device)
    native().gather_rows(out, x.contiguous(), idx, div)
    return out


def moe_grouped_gemm(x: torch.Tensor, w: torch.Tensor, offsets: torch.Tensor, swiglu: bool = False,
                     out: Optional[torch.Tensor] = None, zero_fill: bool = True) -> torch.Tensor:
    """All experts' GEMMs in one launch over expert-sorted rows: ``x`` [rows, K], ``w`` [E, N, K],
    ``offsets`` [E + 1] int32 absolute row offsets of the experts' rows in ``x`` (moe_align, may be
    a slice for this rank's experts).  ``swiglu``: ``w`` is gate/up-interleaved and the result is
    silu(gate) * up [rows, N / 2].  Rows of other experts are left as in ``out`` (zeros when
    allocated here).  GPU: no host synchronisation (gemm_tile.hip 256 x 256 tiles where N % 256 == 0,
    else moe_gemm.hip).  A fragment-packed ``w`` [E, N/16, K/32, 64, 8] (ONE_LAYOUT; ``swiglu=8``:
    the per-16 gate/up pairing) always takes the tile kernel."""
    packed = w.dim() == 5
    N, K = (w.shape[1] * 16, w.shape[2] * 32) if packed else w.shape[1:]
    if out is None:  # zero_fill=False when ``offsets`` covers every row (all experts are local)
        alloc = torch.zeros if zero_fill else torch.empty
        out = alloc(x.shape[0], N // 2 if swiglu else N, dtype=x.dtype, device=x.device)
    epi = _tile_epi(swiglu)
    # the 256 x 256 tile kernel (gemm_tile.hip) where it has whole n-tiles: 1.12-1.15 PF/s on Mixtral's
    # expert shapes against 0.86-0.94 for the 128-tile kernel (profiles/r02/gemm_tile_vs_hipblaslt.jsonl).
    # (The expert count is no part of the routing: past the kernel's limit the binding refuses.)
    if packed or not _gpu(x) or (N % 256 == 0 and tile_form_why("bf16", epi, 1, 0, TILE_ALGO, N, K) is None):
        return _gemm_tile(x, w, None, epi, TILE_ALGO, offsets=offsets, out=out)
    native().moe_grouped_gemm(out, x.contiguous(), w, offsets.contiguous(), swiglu)
    return out


# ---------------------------------------------------------------- the prefill tile GEMM's forms
# The compiled forms of gemm_tile as (weight format, epilogue, grouped, row scale, also at
# schedule 0): the rows of kTileForms in csrc/gemm_tile_forms.h - where the table of accepted
# launches stands, above tile_plan - which native().gemm_tile_forms() reports
# (tests/test_tile_plan_cpu.py compares the two).  Kept here as well because the CPU path refuses
# what the kernel has no form for, with no extension built.
TILE_EPI_BF16, TILE_EPI_SWIGLU, TILE_EPI_ROPE, TILE_EPI_RESID, TILE_EPI_SWIGLU8 = range(5)
TILE_ENCS = ("bf16", "fp8", "mxfp4")  # enc_name(w); the index is the weight format (TILE_W_*)
# kTileFmts, per weight format: (least K, depth of a scale group along K or 0, bits per weight)
TILE_FMTS = ((64, 0, 16), (192, 0, 8), (256, 128, 4))
TILE_SCH1_MIN_K = 192  # schedule 1's peeled ring tail needs three k-tiles; below, bf16 runs schedule 0
TILE_MAX_EXPERTS = 256
TILE_FORMS: tuple = (
    (0, TILE_EPI_BF16, 0, 0, 1),
    (0, TILE_EPI_SWIGLU, 0, 0, 1),
    (0, TILE_EPI_SWIGLU8, 0, 0, 1),
    (0, TILE_EPI_ROPE, 0, 0, 1),
    (0, TILE_EPI_RESID, 0, 0, 0),
    (0, TILE_EPI_SWIGLU, 0, 1, 0),
    (0, TILE_EPI_SWIGLU8, 0, 1, 0),
    (0, TILE_EPI_ROPE, 0, 1, 0),
    (0, TILE_EPI_BF16, 1, 0, 1),
    (0, TILE_EPI_SWIGLU, 1, 0, 1),
    (0, TILE_EPI_SWIGLU8, 1, 0, 1),
) + tuple((fmt, epi, 0, rs, 0) for fmt in (1, 2) for epi, rs in (
    (TILE_EPI_BF16, 0), (TILE_EPI_SWIGLU8, 0), (TILE_EPI_SWIGLU8, 1), (TILE_EPI_ROPE, 0), (TILE_EPI_ROPE, 1),
    (TILE_EPI_RESID, 0)))
# kTilePersist, beside the table: the dense bf16 schedule-1 rows (epi, row scale) that are also
# compiled as a persistent kernel - a grid of min(tiles, CUs) workgroups walking the tiles, the next
# tile's ring fill under the epilogue (csrc/gemm_tile.hip PERSIST) - and whether tile_plan routes a
# launch with more tiles than CUs there by itself (profiles/r23/README.md); native().gemm_tile_persist_forms()
# reports the header's rows (tests/test_tile_persist_cpu.py compares the two).
TILE_PERSIST_FORMS: tuple = ((TILE_EPI_ROPE, 1, 1), (TILE_EPI_RESID, 0, 1), (TILE_EPI_SWIGLU8, 1, 1))
# A/B only (module constants, not environment switches): TILE_PERSIST -1 = as the table routes, 1 = the
# persistent form wherever it is compiled, 0 = nowhere; TILE_PERSIST_CUS: the persistent grid's size, 0 =
# the device's CU count (tests cap it at 3 so that every workgroup crosses a seam on small shapes).
TILE_PERSIST = -1
TILE_PERSIST_CUS = 0
_TILE_EPI_NAMES = ("plain", "swiglu=1 (per-128 pairing)", "RoPE", "residual", "swiglu=8")
# the table by key (every prefill GEMM asks it): row -> has schedule 0; (format, epilogue) pairs; grouped formats
_TILE_SCH0 = {f[:4]: f[4] for f in TILE_FORMS}
_TILE_FMT_EPI = {f[:2] for f in TILE_FORMS}
_TILE_FMT_GROUPED = {f[0] for f in TILE_FORMS if f[2]}


def _tile_epi(swiglu, rope=None) -> int:
    return TILE_EPI_ROPE if rope is not None else TILE_EPI_SWIGLU8 if swiglu == 8 else \
        TILE_EPI_SWIGLU if swiglu else TILE_EPI_BF16


def tile_form_why(enc: str, epi: int, experts: int = 0, rs_np: int = 0, sch: Optional[int] = 1, N: int = 0,
                  K: int = 0, full: bool = True) -> Optional[str]:
    """THE rule of gemm_tile's forms, tile_plan's twin (csrc/gemm_tile_forms.h; tests/test_tile_plan_cpu.py
    sweeps the two against each other): None where TILE_FORMS has a form for a weight in encoding
    ``enc`` [N, K] with epilogue ``epi`` over ``experts`` experts (0: dense), ``rs_np`` row-scale
    partial sums per row (0: no row scale), requested schedule ``sch``; else the reason, as the
    ValueError's text.  ``full=False`` asks only what defines the op - a row of the table, heads and
    partial sums of 128 columns, and (``sch`` not None) that the row has the schedule: what is
    asked for a bf16 weight, whose CPU reference takes any shape and whose launch the binding
    checks against tile_plan; codes are refused here, in full, on the CPU as on the GPU."""
    fmt = TILE_ENCS.index(enc)
    min_k, k_group, bits = TILE_FMTS[fmt]
    grouped, rs = experts != 0, rs_np != 0
    if grouped and fmt not in _TILE_FMT_GROUPED:
        return f"gemm_tile: the {enc}-W form is not compiled for grouped launches"
    if 0 <= epi < len(_TILE_EPI_NAMES) and (fmt, epi) not in _TILE_FMT_EPI:
        return f"gemm_tile: the {enc}-W form is not compiled for {_TILE_EPI_NAMES[epi]} launches"
    sch0 = _TILE_SCH0.get((fmt, epi, int(grouped), int(rs)))
    if sch0 is None:
        return (f"gemm_tile: no {'grouped' if grouped else 'dense'} {enc} form with epilogue {epi}"
                f"{' and a row scale' if rs else ''}: RoPE, the residual epilogue and the row scale are dense, "
                "and the row scale is for the fused consumers (SwiGLU or RoPE)")
    if epi in (TILE_EPI_ROPE, TILE_EPI_RESID) and N % 128:
        return f"gemm_tile: the {_TILE_EPI_NAMES[epi]} epilogue needs N % 128 == 0, not N={N}"
    if sch is not None:
        if fmt and sch != 1:
            return f"gemm_tile: the {enc}-W form is compiled for schedule 1 (algo=1) only, not schedule {sch}"
        if full and sch not in (0, 1):
            return f"gemm_tile: schedule (algo) 0 or 1, not {sch}"
        if (sch != 1 or (full and K < TILE_SCH1_MIN_K)) and not sch0:
            return (f"gemm_tile: the {_TILE_EPI_NAMES[epi]} epilogue{' with a row scale' if rs else ''} needs "
                    f"schedule 1 (algo=1) and K >= {TILE_SCH1_MIN_K}, not schedule {sch} at K={K}")
    if not full:
        return None
    why = None
    if experts < 0 or experts > TILE_MAX_EXPERTS:
        why = f"1..{TILE_MAX_EXPERTS} experts"
    elif rs and (rs_np < 4 or rs_np > 64 or rs_np % 4):
        why = "4..64 row-scale partial sums per row, a multiple of 4"
    elif N % 16 or K % 64 or K < min_k or (k_group and K % k_group):
        why = f"N % 16 == 0, K >= {min_k}, K % {k_group or 64} == 0"
    elif epi in (TILE_EPI_SWIGLU, TILE_EPI_SWIGLU8) and N % 256:
        why = "SwiGLU: N % 256 == 0"
    elif N * K // 8 * bits >= 1 << 31 or 256 * K * 2 >= 1 << 31 or (epi == TILE_EPI_RESID and 256 * N * 2 >= 1 << 31):
        why = "32-bit DMA offsets: the weight, 256 rows of x and of the residual below 2^31 bytes"
    return None if why is None else f"gemm_tile: no {enc} form for N={N} K={K} ({why})"


def tile_f8_ok(N: int, K: int) -> bool:
    """gemm_tile has an fp8-W form for a dense weight [N, K] (schedule 1 only: at least three k-tiles)."""
    return tile_form_why("fp8", TILE_EPI_BF16, N=N, K=K) is None


def tile_f4_ok(N: int, K: int) -> bool:
    """gemm_tile has an mxfp4-W form for a dense weight [N, K] (whole 128-deep scale groups, at least two)."""
    return tile_form_why("mxfp4", TILE_EPI_BF16, N=N, K=K) is None


def tile_codes_ok(w: torch.Tensor) -> bool:
    """gemm_tile has a form that reads the codes tensor ``w`` (tile_f8_ok / tile_f4_ok of its shape)."""
    N, K = skinny_wdims(w)
    return tile_form_why(enc_name(w), TILE_EPI_BF16, N=N, K=K) is None


def _tile_codes_check(w: torch.Tensor, wscale: Optional[torch.Tensor], enc: str) -> None:
    """The tensors of a quantised W of gemm_tile: the codes' layout and the scales that go with them."""
    f4 = enc == "mxfp4"
    if w.dim() != 4 or w.shape[-2:] != (64, 16):
        raise ValueError(f"gemm_tile: an {enc} w is pack_skinny_f{4 if f4 else 8}'s [N/16, K/{128 if f4 else 64}, 64, 16]")
    N, K = skinny_wdims(w)
    shape, dtype = ((N // 16, K // 128, 16, 4), torch.uint8) if f4 else ((N,), torch.float32)
    if wscale is None or wscale.dtype != dtype or (tuple(wscale.shape) != shape if f4 else wscale.numel() != N):
        raise ValueError(f"gemm_tile: an {enc} weight needs its {list(shape)} {dtype} scales")


def _gemm_tile(x: torch.Tensor, w: torch.Tensor, wscale: Optional[torch.Tensor], epi: int, algo: int,
               offsets: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               rope: Optional[tuple] = None, rowscale: Optional[tuple] = None, resid: Optional[torch.Tensor] = None,
               norm_w: Optional[torch.Tensor] = None, hw: Optional[torch.Tensor] = None,
               ss: Optional[torch.Tensor] = None):
    """The one body of gemm_tile, gemm_tile_resid and moe_grouped_gemm's tile launches: the checks
    (tile_form_why), the CPU reference over the decoded W, and THE native().gemm_tile call.
    Returns ``out``, or ``(hw, ss)`` for the residual epilogue."""
    M = x.shape[0]
    grouped, gpu = offsets is not None, _gpu(x)
    enc = "mxfp4" if w.dtype == torch.uint8 else "fp8" if w.dtype == torch.float8_e4m3fn else "bf16"
    quant, swg = enc != "bf16", epi in (TILE_EPI_SWIGLU, TILE_EPI_SWIGLU8)
    packed = w.dim() == (5 if grouped else 4)
    N = w.shape[-4] * 16 if packed else w.shape[-2]
    rs_np = rowscale[0].shape[1] if rowscale is not None else 0
    why = tile_form_why(enc, epi, int(grouped), rs_np, algo if quant or gpu else None, N, x.shape[1], full=quant)
    if why is not None:
        raise ValueError(why)
    if quant:
        _tile_codes_check(w, wscale, enc)
    if epi == TILE_EPI_RESID:
        if resid.shape != (M, N):
            raise ValueError("gemm_tile_resid: resid [M, N]")
        hw = hw if hw is not None else torch.empty_like(resid)
        ss = ss if ss is not None else torch.empty(M, N // 128, dtype=torch.float32, device=resid.device)
    elif out is None:
        alloc = torch.zeros if grouped else torch.empty
        out = alloc(M, N // 2 if swg else N, dtype=x.dtype, device=x.device)
    if gpu:
        pos, cs, heads = rope if rope is not None else (None, None, 0)
        rs_part, rs_eps = rowscale if rowscale is not None else (None, 1e-5)
        native().gemm_tile(y=out if resid is None else resid, x=x.contiguous(), w=w,
                           offsets=offsets.contiguous() if grouped else None,
                           swiglu=8 if epi == TILE_EPI_SWIGLU8 else int(swg), algo=algo, rope_pos=pos, rope_cs=cs,
                           rope_heads=heads, rs_part=rs_part, rs_eps=rs_eps, resid=resid, hw=hw,
                           norm_w=norm_w.contiguous() if norm_w is not None else None, ss_out=ss, wscale=wscale,
                           persist=TILE_PERSIST, cus=TILE_PERSIST_CUS)
        return out if resid is None else (hw, ss)
    if quant:  # the dequantised values: exactly the bf16 encoding's
        w = dequantize_codes(w, wscale, x.dtype)
    elif packed:
        w = torch.stack([unpack_skinny(e) for e in w]) if grouped else unpack_skinny(w)
    inv = None
    if rowscale is not None:
        ssp, eps = rowscale
        inv = torch.rsqrt(ssp[:M].float().sum(1, keepdim=True) / x.shape[1] + eps)

    def one(xr, wr):
        y = torch.nn.functional.linear(xr.float(), wr.float())
        if inv is not None:
            y = y * inv
        y = y.to(x.dtype)
        if epi == TILE_EPI_SWIGLU8:
            g = y.view(y.shape[0], -1, 16)
            return (torch.nn.functional.silu(g[..., :8].float()) * g[..., 8:].float()).reshape(y.shape[0], -1).to(x.dtype)
        return silu_mul(y, interleaved=True) if swg else y
    if epi == TILE_EPI_RESID:
        h = (one(x, w).float() + resid.float()).to(resid.dtype)
        resid.copy_(h)
        hw.copy_((h.float() * norm_w.float()).to(hw.dtype))
        ss.copy_((h.float() ** 2).view(M, N // 128, 128).sum(2))
        return hw, ss
    if grouped:
        off = offsets.tolist()
        for e in range(w.shape[0]):
            a, b = off[e], off[e + 1]
            if b > a:
                out[a:b] = one(x[a:b], w[e])
        return out
    out.copy_(one(x, w))
    if rope is not None:
        pos, cs, heads = rope
        h = out[:, : heads * 128].view(M, heads, 128).float()
        c = cs[pos.long(), :64].float()[:, None]
        s_ = cs[pos.long(), 64:].float()[:, None]
        a, b = h[..., :64], h[..., 64:]
        out[:, : heads * 128] = torch.cat([a * c - b * s_, b * c + a * s_], -1).reshape(M, -1).to(out.dtype)
    return out


def gemm_tile(x: torch.Tensor, w: torch.Tensor, offsets: Optional[torch.Tensor] = None, swiglu: bool = False,
              out: Optional[torch.Tensor] = None, algo: int = 0, rope: Optional[tuple] = None,
              rowscale: Optional[tuple] = None, wscale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Prefill-sized ``x @ w^T`` on the 256 x 256 MFMA tile kernel (csrc/gemm_tile.hip).

    Dense: ``w`` [N, K].  Grouped: ``w`` [E, N, K] and ``offsets`` [E + 1] int32 device offsets of
    each expert's rows in the expert-sorted ``x`` (moe_align; a slice for this rank's experts) - no
    host synchronisation.  ``swiglu``: ``w`` is gate/up-interleaved (interleave_gate_up) and the
    result is silu(gate) * up [M, N / 2].  Grouped rows outside the offsets are left as in ``out``
    (zeros when allocated here).  ``rope = (positions [M] int32, cos_sin [P, 128] fp32, heads)``:
    the epilogue applies rotate-half RoPE (head_dim 128) to output heads 0 .. heads - 1 of each row
    at its position, on the bf16-rounded product.
    ``rowscale = (ss_part [M, K / 128] fp32, eps)``: the deferred half of an RMSNorm - every row of
    the product is multiplied by rsqrt(sum(ss_part[row]) / K + eps) before the epilogue (``x`` holds
    the norm's weighted input, gemm_tile_resid's ``hw``).
    ``w`` may also be fragment-packed (pack_skinny: [N/16, K/32, 64, 8], grouped [E, ...]): the
    decode GEMMs' layout, consumed as is (every W DMA piece one contiguous 1-KiB block).
    ``swiglu=8``: the gate/up rows are interleaved per 16 (interleave_gate_up8, the decode GEMMs'
    SwiGLU copy) instead of per 128 - prefill and decode then share one weight.
    ``w`` may be the fp8 decode encoding (pack_skinny_f8 codes [N/16, K/64, 64, 16]) with ``wscale``
    its [N] fp32 row scales in packed row order, or the mxfp4 one (pack_skinny_f4 codes
    [N/16, K/128, 64, 16] uint8) with ``wscale`` its e8m0 block scales [N/16, K/128, 16, 4] uint8 -
    the tensors gemm_dec streams, converted on the way into the MFMA, bit-identical to the packed
    bf16 form over the dequantised weight.
    Which combinations of these are compiled, and for which N, K and schedule ``algo``: TILE_FORMS
    and tile_form_why here, the table above tile_plan in csrc/gemm_tile_forms.h; any other raises."""
    if rope is not None and swiglu:
        raise ValueError("gemm_tile: one epilogue - SwiGLU or RoPE")
    return _gemm_tile(x, w, wscale, _tile_epi(swiglu, rope), algo, offsets=offsets, out=out, rope=rope,
                      rowscale=rowscale)


def gemm_tile_resid(x: torch.Tensor, w: torch.Tensor, resid: torch.Tensor, norm_w: torch.Tensor,
                    hw: Optional[torch.Tensor] = None, ss: Optional[torch.Tensor] = None,
                    wscale: Optional[torch.Tensor] = None) -> tuple:
    """A residual-producing prefill projection with the next RMSNorm's pass fused into its epilogue
    (csrc/gemm_tile.hip TILE_EPI_RESID; dense, N % 128 == 0): ``resid`` [M, N] <- bf16(resid +
    bf16(x @ w^T)) in place; returns ``(hw, ss)`` - hw = bf16(resid * norm_w) [M, N] and ss [M, N / 128]
    fp32 partial sums of resid^2 over each 128 columns, the operands of the consumer's row scale
    (``gemm_tile(hw, ..., rowscale=(ss, eps))`` = the projection of rms_norm(resid) * norm_w).
    ``w`` row-major, fragment-packed, or the fp8 / mxfp4 encoding with ``wscale`` (see gemm_tile)."""
    return _gemm_tile(x, w, wscale, TILE_EPI_RESID, TILE_ALGO, resid=resid, norm_w=norm_w, hw=hw, ss=ss)


# Prefill projections (qkv / o / gate_up + SwiGLU / down) on the hand-written 4-wave MFMA GEMM
# (csrc/gemm_tile.hip, two-barrier schedule) or hipBLASLt (torch F.linear).  The default ("tile")
# takes the tile kernel for every projection of at least TILE_MIN_M rows: in isolation hipBLASLt is
# 4-8 % faster on o / down (profiles/r03/gemm_ring_addressing.jsonl), but in the served headline
# the all-tile routing measured +1.4 % (three interleaved pairs, profiles/r04/bench_pg2_*.json:
# 25.06 vs 24.71 q/s), with qkv's RoPE fused into the tile epilogue.  "auto" = tile for the fused
# epilogues only (gate_up + SwiGLU, qkv + RoPE), hipBLASLt for o / down; "blas" = hipBLASLt for all.
# These routes apply to row-major weights; the ONE_LAYOUT models' fragment-packed weights (every
# Llama / Mixtral on the GPU) go to the tile kernel at any row count - hipBLASLt cannot read them.
# These are module constants (tools and tests set them for A/B runs), not environment switches.
PREFILL_GEMM = "tile"
QKV_ROPE_TILE = True  # qkv + fused RoPE on the tile kernel
# residual-add RMSNorm folded into the o / down epilogues and the qkv / gate_up row scale
FUSED_NORM = True
TILE_MIN_M = 1024  # below this a 256-row tile wastes most of its MFMAs on padding rows
# 1: the 4-wave kernel's two-barrier schedule, 0: one barrier per k-tile (K < 192 only)
TILE_ALGO = 1


def tile_shape_ok(M: int, N: int, K: int, swiglu: bool = False) -> bool:
    """gemm_tile takes this prefill GEMM (rows, output columns, depth)."""
    return M >= TILE_MIN_M and K >= 128 and tile_form_why("bf16", _tile_epi(swiglu), 0, 0, TILE_ALGO, N, K) is None


def fused_norm_ok(M: int, d: int, n_qkv: int, n_o_in: int, n_13: int, f: int) -> bool:
    """The prefill layer may run with its RMSNorms folded into the tile GEMMs (gemm_tile_resid +
    row scale): every projection on the tile kernel (default routing), qkv with the RoPE epilogue,
    d a multiple of 128 with at most 64 partial sums per row (d <= 8192)."""
    return (FUSED_NORM and PREFILL_GEMM == "tile" and QKV_ROPE_TILE and d % 128 == 0 and d // 128 <= 64
            and n_qkv % 128 == 0 and tile_shape_ok(M, n_qkv, d) and tile_shape_ok(M, d, n_o_in)
            and tile_shape_ok(M, n_13, d, swiglu=True) and tile_shape_ok(M, d, f) and 256 * d * 2 < (1 << 31))


def w_out(w: torch.Tensor) -> int:
    """Output features of a dense projection weight: row-major [N, K], fragment-packed
    [N/16, K/32, 64, 8] (pack_skinny), the fp8 encoding [N/16, K/64, 64, 16] (pack_skinny_f8) or the
    mxfp4 one [N/16, K/128, 64, 16] (pack_skinny_f4)."""
    return w.shape[0] * 16 if w.dim() == 4 else w.shape[0]


def w_in(w: torch.Tensor) -> int:
    """Input features (K) of a row-major, fragment-packed, fp8- or mxfp4-encoded dense projection weight."""
    return skinny_wdims(w)[1]


def prefill_linear(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False,
                   out: Optional[torch.Tensor] = None, rope: Optional[tuple] = None,
                   rowscale: Optional[tuple] = None, wscale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x @ w^T`` for a prefill-sized ``x`` [M, K] and row-major ``w`` [N, K]; ``swiglu``: ``w`` is
    gate/up-interleaved (interleave_gate_up) and the result is silu(gate) * up [M, N / 2] - fused
    into the tile kernel's epilogue, or F.linear + silu_mul on the library path.
    ``rope = (positions, cos_sin, heads)`` (the qkv projection, head_dim 128): the tile kernel
    rotates heads 0 .. heads - 1 in its epilogue; returns ``(y, rotated)`` - rotated False when the
    library took the GEMM (the caller then applies RoPE itself).
    A fragment-packed ``w`` (pack_skinny, the ONE_LAYOUT resident form; ``swiglu=8`` with the
    interleave_gate_up8 pairing) always takes the tile kernel, whatever the row count - hipBLASLt
    cannot read it; on the CPU gemm_tile unpacks it for the fp32 reference.  So does the fp8
    encoding of a weight (pack_skinny_f8 codes with ``wscale``, where the model keeps no bf16 copy)
    and the mxfp4 one (pack_skinny_f4 codes with ``wscale`` their block scales)."""
    M, K = x.shape
    if w.dim() == 4:
        ws = wscale if is_fp8(w) or is_mxfp4(w) else None
        if rope is not None:
            return gemm_tile(x, w, out=out, algo=TILE_ALGO, rope=rope, rowscale=rowscale, wscale=ws), True
        return gemm_tile(x, w, swiglu=swiglu, out=out, algo=TILE_ALGO, rowscale=rowscale, wscale=ws)
    N = w.shape[0]
    mode = PREFILL_GEMM
    tile_ok = _gpu(x) and tile_shape_ok(M, N, K, swiglu)
    if rope is not None:
        # the qkv projection takes the tile kernel whenever its RoPE epilogue applies: it replaces
        # rope_cache's read-rotate-write pass over q / k (more than the GEMM gives up to hipBLASLt)
        if (tile_ok and N % 128 == 0 and mode != "blas" and QKV_ROPE_TILE) or rowscale is not None:
            return gemm_tile(x, w, out=out, algo=TILE_ALGO, rope=rope, rowscale=rowscale), True
        return prefill_linear(x, w, out=out), False
    if rowscale is not None:  # the fused-norm consumer (the caller checked fused_norm_ok)
        return gemm_tile(x, w, swiglu=swiglu, out=out, algo=TILE_ALGO, rowscale=rowscale)
    use_tile = tile_ok and (mode == "tile" or (mode == "auto" and swiglu))
    if use_tile:
        return gemm_tile(x, w, swiglu=swiglu, out=out, algo=TILE_ALGO)
    y = torch.nn.functional.linear(x, w)
    if swiglu:
        return silu_mul(y, out=out, interleaved=True)
    return out.copy_(y) if out is not None else y


def moe_combine(y: torch.Tensor, inv_idx: torch.Tensor, w: torch.Tensor, T: int) -> torch.Tensor:
    if not _gpu(y):
        return ref.moe_combine(y, inv_idx, w, T)
    out = torch.empty(T, y.shape[1], dtype=y.dtype, device=y.device)
    native().moe_combine(out, y.contiguous(), inv_idx, w.contiguous())
    return out


def softmax_scale(head_dim: int) -> float:
    return 1.0 / math.sqrt(head_dim)
