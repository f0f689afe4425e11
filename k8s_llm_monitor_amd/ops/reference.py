"""Plain-PyTorch fp32 references of every fused op (fp64 inside rms_norm, silu_mul and moe_combine,
where a chain of fp32 roundings or fp32's range would show in the bf16 result).

They define the semantics the HIP kernels must reproduce (tests compare the two), and they
are the execution path for CPU tensors (unit tests, the GPT-2 CPU plumbing config).
KV-cache layouts (see ``csrc/rope_cache.hip``):

* ``k_cache`` ``[num_blocks, Hkv, D // 8, block_size, 8]``
* ``v_cache`` ``[num_blocks, Hkv, D, block_size]``, each block's tokens at positions ``v_perm(t)``
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    # fp64: the fp32 sum of squares loses the small terms of a row that holds an outlier, and the
    # chain of fp32 roundings after it is visible at a bf16 rounding boundary
    # (tests/test_small_ops_models_cpu.py holds every reference to one fp32 rounding)
    xf = x.double()
    eps32 = float(torch.tensor(eps, dtype=torch.float32))  # the kernel's eps is an fp32 argument
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps32) * w.double()
    return y.to(x.dtype)


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float):
    s = (x.float() + residual.float()).to(x.dtype)
    return rms_norm(s, w, eps), s


def layer_norm(x, w, b, eps):
    return F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps).to(x.dtype)


def silu_mul(x: torch.Tensor, interleaved: bool = False, pairing: int | None = None) -> torch.Tensor:
    """silu(gate) * up; ``interleaved``: columns are [64 gate | 64 up] per 128.  ``pairing`` says the
    same as a number and knows one more form: 0 [F gate | F up], 1 per 128 columns, 8 [8 gate | 8 up]
    per 16 columns (the row order of ops.interleave_gate_up8)."""
    f = x.shape[-1] // 2
    xf = x.double()  # fp32 loses silu(gate) below -88 (exp overflows) while silu(gate) * up is still normal
    if pairing is None:
        pairing = 1 if interleaved else 0
    if pairing not in (0, 1, 8):
        raise ValueError(f"silu_mul: pairing {pairing!r} is not 0, 1 or 8")
    if pairing:
        w = 64 if pairing == 1 else 8
        t = xf.reshape(*xf.shape[:-1], f // w, 2, w)
        return (F.silu(t[..., 0, :]) * t[..., 1, :]).reshape(*xf.shape[:-1], f).to(x.dtype)
    return (F.silu(xf[..., :f]) * xf[..., f:]).to(x.dtype)


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    return F.gelu(x.float(), approximate="tanh").to(x.dtype)


def embedding(ids: torch.Tensor, weight: torch.Tensor, vocab_start: int = 0) -> torch.Tensor:
    local = ids.long() - vocab_start
    ok = (local >= 0) & (local < weight.shape[0])
    out = weight[local.clamp(0, weight.shape[0] - 1)]
    return out * ok.unsqueeze(-1).to(out.dtype)


def rope_cos_sin(max_pos: int, head_dim: int, theta: float, scaling: dict | None = None,
                 device=None) -> torch.Tensor:
    """[max_pos, head_dim] fp32 table: first half cos, second half sin (neox pairing).

    ``scaling`` supports the Llama-3.1 ``{"rope_type": "llama3", "factor", "low_freq_factor",
    "high_freq_factor", "original_max_position_embeddings"}`` frequency remap.
    """
    half = head_dim // 2
    inv = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64) * 2 / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        lo, hi = scaling["low_freq_factor"], scaling["high_freq_factor"]
        orig = scaling["original_max_position_embeddings"]
        wavelen = 2 * math.pi / inv
        lo_wl, hi_wl = orig / lo, orig / hi
        smooth = (orig / wavelen - lo) / (hi - lo)
        scaled = torch.where(wavelen > lo_wl, inv / factor, inv)
        mid = (wavelen <= lo_wl) & (wavelen >= hi_wl)
        inv = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
    t = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(t, inv)
    return torch.cat([ang.cos(), ang.sin()], dim=-1).float().to(device)


def apply_rope(x: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """x: [T, H, D]; returns rotated fp32 (fp64 for an fp64 ``x``)."""
    d = x.shape[-1]
    half = d // 2
    cs = cos_sin[positions.long()]
    c, s = cs[:, None, :half], cs[:, None, half:]
    xf = x if x.dtype == torch.float64 else x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def head_rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """QK-norm: x [T, H, D] RMS-normalised over D and scaled by w [D]; fp32."""
    xf = x.float()
    r = torch.rsqrt(xf.square().sum(-1, keepdim=True) * (1.0 / x.shape[-1]) + eps)
    return xf * r * w.float()


def rope_and_cache(qkv, positions, cos_sin, k_cache, v_cache, slot_mapping, Hq, Hkv, D, apply_rope_=True,
                   kv_scale=None, qk_norm=None):
    """``qk_norm = (q_w, k_w, eps)``: each q / k head RMS-normalised over D and scaled by its
    weight in fp32, in the kernel's order (x * rsqrt(mean(x^2) + eps) * w), before the rotation;
    one rounding to ``qkv.dtype`` at the end."""
    T = qkv.shape[0]
    q = qkv[:, : Hq * D].view(T, Hq, D)
    k = qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
    v = qkv[:, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D].view(T, Hkv, D)
    if qk_norm is not None:
        q_w, k_w, eps = qk_norm
        qn, kn = head_rms_norm(q, q_w, eps), head_rms_norm(k, k_w, eps)
        if apply_rope_:
            qn, kn = apply_rope(qn, positions, cos_sin), apply_rope(kn, positions, cos_sin)
        q.copy_(qn.to(qkv.dtype))
        k.copy_(kn.to(qkv.dtype))
    elif apply_rope_:
        q.copy_(apply_rope(q, positions, cos_sin).to(qkv.dtype))
        k.copy_(apply_rope(k, positions, cos_sin).to(qkv.dtype))
    if slot_mapping is not None and slot_mapping.numel() > 0:
        write_kv_cache(k, v, k_cache, v_cache, slot_mapping, kv_scale)


def v_perm(t):
    """V-cache position of block token t (common.h v_perm): bits 2 and 3 swapped, an involution."""
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def _kv_is_fp8(k_cache) -> bool:
    return k_cache.dtype == torch.float8_e4m3fn


def write_kv_cache(k, v, k_cache, v_cache, slot_mapping, kv_scale=None):
    """k, v [T, Hkv, D] into the paged cache at ``slot_mapping`` (-1: no write).  An e4m3 cache
    (``kv_scale`` [NB, Hkv, 2, bs]) takes ops.quantize_kv's codes and scales; nothing else moves."""
    bs = k_cache.shape[3]
    D = v_cache.shape[2]
    sm = slot_mapping.long()
    ok = sm >= 0
    sm, k, v = sm[ok], k[ok], v[ok]
    blk, off = sm // bs, sm % bs
    if _kv_is_fp8(k_cache):
        from . import quantize_kv
        (kq, ks), (vq, vs) = quantize_kv(k), quantize_kv(v)
        k_cache.view(torch.uint8)[blk, :, :, off, :] = kq.view(torch.uint8).view(k.shape[0], k.shape[1], D // 8, 8)
        v_cache.view(torch.uint8)[blk, :, :, v_perm(off)] = vq.view(torch.uint8)
        kv_scale[blk, :, 0, off] = ks
        kv_scale[blk, :, 1, off] = vs
        return
    kk = k.view(k.shape[0], k.shape[1], D // 8, 8)
    k_cache[blk, :, :, off, :] = kk
    v_cache[blk, :, :, v_perm(off)] = v


def gather_kv(k_cache, v_cache, block_table: torch.Tensor, seq_len: int, kv_scale=None):
    """Contiguous [L, Hkv, D] keys and values of one sequence (an e4m3 cache: dequantised, bf16)."""
    bs = k_cache.shape[3]
    nb = (seq_len + bs - 1) // bs
    blocks = block_table[:nb].long()
    if _kv_is_fp8(k_cache):
        from . import dequantize_kv
        kq, vq = gather_kv(k_cache.view(torch.uint8), v_cache.view(torch.uint8), block_table, seq_len)
        sc = kv_scale[blocks].permute(2, 0, 3, 1).reshape(2, nb * bs, -1)[:, :seq_len]  # [2, L, Hkv]
        return (dequantize_kv(kq.view(torch.float8_e4m3fn), sc[0]), dequantize_kv(vq.view(torch.float8_e4m3fn), sc[1]))
    kb = k_cache[blocks]  # [nb, Hkv, D/8, bs, 8]
    nbk, hkv, p, _, _ = kb.shape
    k = kb.permute(0, 3, 1, 2, 4).reshape(nbk * bs, hkv, p * 8)[:seq_len]
    vb = v_cache[blocks]  # [nb, Hkv, D, bs], tokens at positions v_perm(t)
    vb = vb[..., v_perm(torch.arange(bs, device=vb.device))]
    v = vb.permute(0, 3, 1, 2).reshape(nbk * bs, hkv, -1)[:seq_len]
    return k, v


def attention(q, k, v, scale: float, causal: bool) -> torch.Tensor:
    """q [Tq, Hq, D], k/v [Tk, Hkv, D] (GQA broadcast); fp32 result [Tq, Hq, D].
    causal aligns the last query with the last key."""
    hq, hkv = q.shape[1], k.shape[1]
    g = hq // hkv
    qf = q.float().transpose(0, 1)
    kf = k.float().repeat_interleave(g, dim=1).transpose(0, 1)
    vf = v.float().repeat_interleave(g, dim=1).transpose(0, 1)
    s = qf @ kf.transpose(1, 2) * scale
    if causal:
        tq, tk = q.shape[0], k.shape[0]
        mask = torch.ones(tq, tk, dtype=torch.bool, device=q.device).tril(tk - tq)
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return (p @ vf).transpose(0, 1)


def paged_decode(q, k_cache, v_cache, block_tables, seq_lens, Hq, Hkv, D, scale, kv_scale=None):
    """q [B, >=Hq*D]; returns [B, Hq*D] in q.dtype."""
    B = seq_lens.shape[0]
    out = torch.zeros(B, Hq * D, dtype=q.dtype, device=q.device)
    for b in range(B):
        L = int(seq_lens[b])
        if L <= 0:
            continue
        k, v = gather_kv(k_cache, v_cache, block_tables[b], L, kv_scale)
        qb = q[b, : Hq * D].view(1, Hq, D)
        out[b] = attention(qb, k, v, scale, causal=False).reshape(-1).to(q.dtype)
    return out


def flash_prefill(qkv, cu_seqlens, Hq, Hkv, D, scale):
    T = qkv.shape[0]
    out = torch.empty(T, Hq * D, dtype=qkv.dtype, device=qkv.device)
    cu = cu_seqlens.tolist()
    for i in range(len(cu) - 1):
        a, b = cu[i], cu[i + 1]
        if b <= a:
            continue
        x = qkv[a:b]
        q = x[:, : Hq * D].view(b - a, Hq, D)
        k = x[:, Hq * D:(Hq + Hkv) * D].view(b - a, Hkv, D)
        v = x[:, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D].view(b - a, Hkv, D)
        out[a:b] = attention(q, k, v, scale, causal=True).reshape(b - a, -1).to(qkv.dtype)
    return out


def paged_prefill(qkv, cu_seqlens, ctx_start, k_cache, v_cache, block_tables, Hq, Hkv, D, scale, kv_scale=None):
    """Queries = each sequence's new rows of ``qkv``; keys/values = positions [0, ctx_start + new)
    from the paged cache (which already holds the new tokens).  An e4m3 cache gives only the
    cached prefix (dequantised): this step's own keys / values are the unquantised qkv rows."""
    T = qkv.shape[0]
    out = torch.empty(T, Hq * D, dtype=qkv.dtype, device=qkv.device)
    cu, cs = cu_seqlens.tolist(), ctx_start.tolist()
    for i in range(len(cu) - 1):
        a, b = cu[i], cu[i + 1]
        if b <= a:
            continue
        k, v = gather_kv(k_cache, v_cache, block_tables[i], cs[i] + b - a, kv_scale)
        if _kv_is_fp8(k_cache):
            k = torch.cat([k[:cs[i]].float(), qkv[a:b, Hq * D:(Hq + Hkv) * D].reshape(b - a, Hkv, D).float()])
            v = torch.cat([v[:cs[i]].float(), qkv[a:b, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D].reshape(b - a, Hkv, D).float()])
        q = qkv[a:b, : Hq * D].view(b - a, Hq, D)
        out[a:b] = attention(q, k, v, scale, causal=True).reshape(b - a, -1).to(qkv.dtype)
    return out


def greedy(logits: torch.Tensor) -> torch.Tensor:
    return logits.float().argmax(-1).to(torch.int32)


def sample_keep(logits_row: torch.Tensor, temperature: float, top_k: int, top_p: float) -> torch.Tensor:
    """bool[V]: the tokens of one row a sampled draw (temperature > 0) may return, in float64.

    Scale by 1/T; top-k keeps {v >= k-th largest v} when 0 < k < V; top-p (p < 1) then takes the
    softmax of the top-k survivors, sorted descending, and keeps the smallest prefix whose mass
    reaches p (``cumsum - p_i < p``).  Ties at the last kept value are kept by both filters, the
    largest value is always kept, and -inf entries never are."""
    v = logits_row.detach().to(torch.float64) * (1.0 / float(temperature))
    keep = v > float("-inf")
    k = int(top_k)
    if 0 < k < v.numel():
        keep &= v >= torch.topk(v, k).values[-1]
    if float(top_p) < 1.0:
        w = torch.softmax(v.masked_fill(~keep, float("-inf")), -1)
        sw = torch.sort(w, descending=True).values
        past = torch.nonzero(~(torch.cumsum(sw, 0) - sw < float(top_p)))
        n = int(past[0]) if past.numel() else sw.numel()  # length of the kept prefix
        keep &= w >= sw[max(n, 1) - 1]
    return keep


def penalty_inv_rep(rep: float) -> float:
    """fp32(1 / rep): computed once on the host, so the kernels and the reference multiply positive
    logits by the same number."""
    return float(torch.tensor(1.0 / float(rep), dtype=torch.float32))


def apply_penalties(logits_row: torch.Tensor, prompt_seen: torch.Tensor, out_count: torch.Tensor, rep: float,
                    presence: float, frequency: float) -> torch.Tensor:
    """fp32[V]: one row of logits after the sampling penalties, every step rounded to fp32.

    1. repetition (HF / vLLM rule, over prompt and output tokens): a token with ``prompt_seen`` or
       ``out_count > 0`` has its logit multiplied by ``fp32(1 / rep)`` when positive, by ``rep``
       otherwise (``rep > 0``, 1 is neutral);
    2. frequency and presence (OpenAI rule, over output tokens only):
       ``x - frequency * out_count - presence * (out_count > 0)``.

    The sampler's pipeline (greedy argmax, or / T, top-k, top-p, the draw) runs on the result."""
    f32 = torch.float32
    x = logits_row.detach().to(f32)
    cnt = out_count.to(torch.int64)
    rep_t = torch.tensor(float(rep), dtype=f32)
    inv_rep = torch.tensor(penalty_inv_rep(rep), dtype=f32)
    hit = prompt_seen.to(torch.bool) | (cnt > 0)
    x = torch.where(hit, torch.where(x > 0, x * inv_rep, x * rep_t), x)
    x = x - torch.tensor(float(frequency), dtype=f32) * cnt.to(f32)
    return x - torch.tensor(float(presence), dtype=f32) * (cnt > 0).to(f32)


def token_logprobs(logits_row: torch.Tensor, token: int, n: int):
    """``(lp, ids[n], lps[n])`` of one row of logits, in fp32.

    ``lp = x[token] - lse`` over the logits as given (``float()``): the model's distribution,
    before penalties, temperature and top-k / top-p; NaN for a token outside ``[0, V)``.  ``ids``
    (int32) are the ``n`` largest logits in the order (value descending, index ascending) - a
    stable descending sort - and ``lps`` (fp32) their log-probabilities; entries past
    ``min(n, V)`` are id -1, logprob -inf."""
    x = logits_row.detach().float()
    V = x.numel()
    lps_all = torch.log_softmax(x, -1)
    t = int(token)
    lp = float(lps_all[t]) if 0 <= t < V else float("nan")
    ids = torch.full((n,), -1, dtype=torch.int32)
    lps = torch.full((n,), float("-inf"), dtype=torch.float32)
    k = min(n, V)
    if k > 0:
        order = torch.sort(x, descending=True, stable=True).indices[:k]
        ids[:k] = order.to(torch.int32)
        lps[:k] = lps_all[order]
    return lp, ids, lps


def guide_advance(trans, state: int, token_bytes: bytes) -> int:
    """The DFA state after walking ``token_bytes`` from ``state`` over ``trans`` ``[n, 256]``
    (-1 = dead); -1 as soon as a transition is dead."""
    s = int(state)
    for b in token_bytes:
        if s < 0:
            return -1
        s = int(trans[s][b])
    return s


def guide_mask(trans, accept, vocab_bytes, eos_ids) -> torch.Tensor:
    """bool ``[n, V]``: the tokens a guided row in DFA state ``s`` may draw.

    Bit ``(s, t)`` is set iff token ``t`` has at least one byte and walking its bytes from ``s``
    never hits -1; for ``t`` in ``eos_ids`` it is set iff ``accept[s]``.  Tokens without bytes are
    never allowed.  All states walk a token position together (one gather per byte position)."""
    import numpy as np

    tr = np.asarray(trans).astype(np.int64)
    n, V = tr.shape[0], len(vocab_bytes)
    ext = np.concatenate([np.where(tr < 0, n, tr), np.full((1, 256), n, dtype=np.int64)])  # row n: dead
    lens = np.array([len(b) for b in vocab_bytes], dtype=np.int64)
    width = int(lens.max()) if V else 0
    tb = np.zeros((V, max(width, 1)), dtype=np.int64)
    for t, b in enumerate(vocab_bytes):
        tb[t, : len(b)] = list(b)
    cur = np.repeat(np.arange(n, dtype=np.int64)[:, None], V, axis=1)
    for j in range(width):
        live = np.flatnonzero(lens > j)
        cur[:, live] = ext[cur[:, live], tb[live, j][None, :]]
    ok = (cur < n) & (lens > 0)[None, :]
    acc = np.asarray(accept).astype(bool)
    for t in eos_ids:
        if 0 <= int(t) < V:
            ok[:, int(t)] = acc
    return torch.from_numpy(ok)


def moe_route(logits: torch.Tensor, k: int, renorm: bool):
    p = torch.softmax(logits.float(), dim=-1)
    w, ids = torch.topk(p, k, dim=-1)
    if renorm:
        w = w / w.sum(-1, keepdim=True)
    return ids.to(torch.int32), w


def moe_align(ids: torch.Tensor, E: int):
    flat = ids.reshape(-1).long()
    order = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=E)
    offsets = torch.zeros(E + 1, dtype=torch.int32, device=ids.device)
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel(), device=ids.device)
    return offsets, order.to(torch.int32), inv.to(torch.int32)


def moe_combine(y: torch.Tensor, inv_idx: torch.Tensor, w: torch.Tensor, T: int) -> torch.Tensor:
    K = w.shape[1]
    g = y.double()[inv_idx.long()].view(T, K, -1)  # K products and their sum, rounded once
    return (g * w.double().unsqueeze(-1)).sum(1).to(y.dtype)


def pool_l2(x: torch.Tensor, dim, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Last-token pooling of embedding requests: row ``r`` of ``x`` [R, d] cut to its first
    ``dim[r]`` columns and L2-normalised (fp64 inside), zeros beyond them; an all-zero row gives
    zeros.  Rows with ``dim[r] <= 0`` are not embedding rows: their ``out`` rows stay as they are
    (zeros in a fresh ``out``).  Returns ``out``, fp32 [R, d]."""
    R, d = x.shape
    if out is None:
        out = torch.zeros(R, d, dtype=torch.float32, device=x.device)
    for r, n in enumerate(torch.as_tensor(dim).reshape(-1)[:R].tolist()):
        if n <= 0:
            continue
        v = x[r, :n].double()
        nrm = v.norm()
        out[r, :n] = (v / nrm if float(nrm) > 0 else torch.zeros_like(v)).float()
        out[r, n:] = 0
    return out


def lora_delta(x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scaling: torch.Tensor, slot: torch.Tensor,
               dtype=torch.float32) -> torch.Tensor:
    """Per-row low-rank adapter delta ``scaling[s] * B[s] @ (A[s] @ x[row])``, ``s = slot[row]``; rows
    with ``slot < 0`` have no adapter and give exact zeros.  ``x`` [M, K], ``A`` [slots, R, K], ``B``
    [slots, N, R], ``scaling`` [slots], ``slot`` [M] integers; computed in ``dtype`` (fp32; the tests
    ask for fp64) one row at a time, so a row's result never depends on the other rows' slots."""
    M, N = x.shape[0], B.shape[1]
    out = torch.zeros(M, N, dtype=dtype, device=x.device)
    sl = slot[:M].tolist()
    conv: dict = {}
    for i, s in enumerate(sl):
        if s < 0:
            continue
        if s not in conv:
            conv[s] = (A[s].to(dtype), B[s].to(dtype), scaling[s].to(dtype))
        a, b, sc = conv[s]
        out[i] = sc * (b @ (a @ x[i].to(dtype)))
    return out
