"""The pre-activation delta of gemm_dec_kernel's SwiGLU epilogue (ops.dec_gemm(.., delta=..)): the
adapters' gate_up delta enters between the accumulator and the activation.

Shapes: F in {160, 1024} (N = 2F: 20 and 128 n-tiles - with 7- or 8-wave workgroups the last
workgroup is ragged in both), K in {512, 1536}, the three SwiGLU forms (1, 1, 7, 8), (1, 1, 7, 16),
(1, 1, 8, 16), M in {1, 15, 16, 17, 64} plus {65, 128} on the form of 8 m-tiles; bf16 weights, and
fp8 / mxfp4 on the forms DEC_F8_FORMS / DEC_F4_FORMS hold; with and without the deferred norm; slot
patterns all -1, all one adapter, (-1, 0, 1, 2) cycling, and the cycle with one slot equal to the
arena's size (out of range = no adapter).

Weight row r (canonical) is scaled by 2^(r % 3 - 1) and the delta's column with it, so neighbouring
columns carry different fp8 scales and the delta has the pre-activations' magnitude: a dropped or
shifted delta fails by orders of magnitude.

Bounds (derived, not tuned; U8 = 2^-8 one bf16 rounding, U24 = 2^-24 one fp32 rounding).
  isolated (x = 0): out = bf16(silu(bf16(d_gate)) * bf16(d_up)) evaluated in fp32:
      |err| <= U8 |ref| + 2^-20 |ref|.
  general: the kernel rounds g and u to bf16 before the activation, so with
      e_g = U8 |g| + (K + 8) U24 (|x| . |W_g|) s + U24 |g|   (s the deferred-norm row scale), likewise e_u,
      |err| <= U8 |ref| + 1.1 |u| e_g + |silu(g)| e_u + 1.1 e_g e_u       (|silu'| <= 1.1).
"""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F_ = torch.nn.functional
U8, U24 = 2.0 ** -8, 2.0 ** -24
EPS = 1e-5
NSLOTS = 3
GUARD = 64
CFGS = [(1, 1, 7, 8), (1, 1, 7, 16), (1, 1, 8, 16)]
PATTERNS = ("none", "same1", "cycle", "oor")


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    for c in (_w, _x, _ss, _delta, _pre):
        c.cache_clear()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _encs(cfg):
    form = (ops.DEC_SWIGLU8,) + tuple(cfg[1:])
    e = ["bf16"]
    if any(ops.DEC_FORMS[i][:4] == form for i in ops.DEC_F8_FORMS):
        e.append("fp8")
    if ops.dec_f4_depth(ops.DEC_SWIGLU8, cfg):
        e.append("mxfp4")
    return e


def _max_m(cfg):
    form = (ops.DEC_SWIGLU8,) + tuple(cfg[1:])
    return max(16 * f[4] for f in ops.DEC_FORMS if f[:4] == form)


def _colscale(F):
    """The scale of canonical weight row r (and of the delta's column that belongs to it)."""
    return torch.exp2((torch.arange(2 * F, device=DEV) % 3 - 1).float())


@functools.lru_cache(maxsize=None)
def _w(F, K, enc):
    """(the weight's values in the packed [8 gate | 8 up] row order [2F, K] bf16, what dec_gemm
    streams, its scales or None, the bf16 packing of the same values)."""
    gu = (torch.randn(2 * F, K, device=DEV, generator=_gen(F * 13 + K)) / K ** 0.5 * _colscale(F)[:, None]).to(torch.bfloat16)
    if enc == "bf16":
        il = ops.interleave_gate_up8(gu).contiguous()
        wp = ops.pack_skinny(il)
        return il, wp, None, wp
    deq, qp, s = ops.encode_weight(gu, enc, gate_up8=True, settle=True)
    il = ops.interleave_gate_up8(deq).contiguous()
    return il, qp, s, ops.pack_skinny(il)


@functools.lru_cache(maxsize=None)
def _x(M, K):
    return torch.randn(M, K, device=DEV, generator=_gen(M * 7919 + K)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _ss(M, K):
    return (torch.rand(M, K // 512, device=DEV, generator=_gen(M + K)) + 0.25) * (K / 2)


@functools.lru_cache(maxsize=None)
def _delta(M, F):
    """fp32 [M, 2F] in the packed row order, of the pre-activations' magnitude."""
    d = torch.randn(M, 2 * F, device=DEV, generator=_gen(M * 31 + F)) * _colscale(F)[None, :]
    return ops.interleave_gate_up8(d.t().contiguous()).t().contiguous()


@functools.lru_cache(maxsize=None)
def _pre(F, K, M, enc):
    """fp64, packed order: (x . W^T, |x| . |W|^T) - shared by every case of the shape, never written."""
    il = _w(F, K, enc)[0].double()
    x = _x(M, K).double()
    return x @ il.t(), x.abs() @ il.abs().t()


def _slots(pattern, M):
    if pattern == "none":
        v = [-1] * M
    elif pattern == "same1":
        v = [1] * M
    else:
        v = [(-1, 0, 1, 2)[(i + 1) % 4] for i in range(M)]  # row 0 has an adapter
        if pattern == "oor":
            v[0 if M < 3 else 2] = NSLOTS  # outside the arena: no adapter
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _launch(F, K, M, cfg, enc, norm, delta=None, slot=None, over_bf16=False):
    """One launch into a guarded output; returns (rows [M, F] bf16 un-packed, the whole guarded buffer)."""
    _, w, s, wp = _w(F, K, enc)
    if over_bf16:
        w, s = wp, None
    MT = -(-M // 16)
    n = MT * (F // 32) * 64 * 8
    buf = ((torch.arange(n + 2 * GUARD, device=DEV) % 251).float() - 125.0).to(torch.bfloat16)
    act = buf[GUARD:GUARD + n].view(MT, F // 32, 64, 8)
    kw = {} if delta is None else dict(delta=delta, delta_slot=slot, delta_slots=NSLOTS)
    ops.dec_gemm(ops.pack_activation(_x(M, K)), w, ops.DEC_SWIGLU8, M, out=act, rownorm=(_ss(M, K), EPS) if norm else None,
                 cfg=cfg, wscale=s, **kw)
    return ops.unpack_skinny(act)[:M], buf


def _guarded(t):
    """A 16-byte aligned copy of ``t`` (fp32) between guard words; (the view, the whole buffer)."""
    buf = (torch.arange(t.numel() + 2 * GUARD, device=DEV) % 241).float() + 1000.0
    v = buf[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 0
    return v, buf


def _deil(t):
    """Packed column order -> [F gate | F up]."""
    return ops.deinterleave_gate_up8(t.t().contiguous()).t()


CASES = [(F, K, cfg, M) for F in (160, 1024) for K in (512, 1536) for cfg in CFGS
         for M in (1, 15, 16, 17, 64, 65, 128) if M <= _max_m(cfg)]


@pytest.mark.parametrize("F,K,cfg,M", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_delta_general(F, K, cfg, M):
    for enc in _encs(cfg):
        acc, mag = _pre(F, K, M, enc)
        for norm in (False, True):
            sc = torch.rsqrt(_ss(M, K).double().sum(1, keepdim=True) / K + EPS) if norm else torch.ones(M, 1, device=DEV, dtype=torch.float64)
            plain, _ = _launch(F, K, M, cfg, enc, norm)
            for pattern in PATTERNS:
                slot = _slots(pattern, M)
                on = (slot >= 0) & (slot < NSLOTS)
                delta, dbuf = _guarded(_delta(M, F))
                dwant = dbuf.clone()
                y, buf = _launch(F, K, M, cfg, enc, norm, delta, slot)
                what = f"F={F} K={K} cfg={cfg} M={M} {enc} norm={norm} {pattern}"
                # guards around out and around delta, delta itself
                n = buf.numel() - 2 * GUARD
                ref_buf = ((torch.arange(n + 2 * GUARD, device=DEV) % 251).float() - 125.0).to(torch.bfloat16)
                assert torch.equal(buf[:GUARD], ref_buf[:GUARD]) and torch.equal(buf[GUARD + n:], ref_buf[GUARD + n:]), what
                assert torch.equal(dbuf, dwant), what + ": delta or its guard words changed"
                # fp64 reference and the composed bound
                pre = acc * sc + delta.double() * on[:, None]
                gu = _deil(pre)
                m2 = _deil(mag * sc)
                g, u = gu[:, :F], gu[:, F:]
                e_g = U8 * g.abs() + (K + 8) * U24 * m2[:, :F] + U24 * g.abs()
                e_u = U8 * u.abs() + (K + 8) * U24 * m2[:, F:] + U24 * u.abs()
                ref = F_.silu(g) * u
                bound = U8 * ref.abs() + 1.1 * u.abs() * e_g + F_.silu(g).abs() * e_u + 1.1 * e_g * e_u
                err = (y.double() - ref).abs()
                print(f"{what}: max err {err.max().item():.3e} max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
                assert bool((err <= bound).all()), what
                # rows without an adapter: the bits of the launch without delta
                assert torch.equal(y[~on], plain[~on]), what + ": a row without an adapter differs from the plain launch"
                if bool(on.any()):
                    assert not torch.equal(y[on], plain[on]), what + ": the delta changed nothing"
                # determinism
                y2, buf2 = _launch(F, K, M, cfg, enc, norm, delta, slot)
                assert torch.equal(buf, buf2), what + ": two launches differ"
                # encodings: the same bits as the bf16 launch over the dequantised weights
                if enc != "bf16":
                    yb, _ = _launch(F, K, M, cfg, enc, norm, delta, slot, over_bf16=True)
                    assert torch.equal(y, yb), what + f": the {enc} launch differs from the bf16 launch over its values"


@pytest.mark.parametrize("F,K,cfg,M", [c for c in CASES if c[1] == 512],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_delta_indexing_isolated(F, K, cfg, M):
    """x = 0: the output is the activation of the delta alone, a distinct value per (row, n)."""
    N = 2 * F
    row = torch.arange(M, device=DEV)[:, None]
    col = torch.arange(N, device=DEV)[None, :]
    # (row, n) -> a bijection of its index on [0, 2^18) (an odd multiplier), so every value in
    # [0.5, 1.5) is exact in fp32 and distinct, and neighbours in n, in rows and in n-tiles are far
    # apart even after the bf16 rounding
    assert M * N <= 1 << 18
    val = 0.5 + (((row * N + col) * 40503) % (1 << 18)).float() / (1 << 18)
    d0 = torch.where((row + col) % 2 == 0, val, -val)
    assert d0.unique().numel() == M * N
    x0 = ops.pack_activation(torch.zeros(M, K, device=DEV, dtype=torch.bfloat16))
    for enc in _encs(cfg):
        _, w, s, _ = _w(F, K, enc)
        for norm in (False, True):
            for pattern in PATTERNS:
                slot = _slots(pattern, M)
                on = (slot >= 0) & (slot < NSLOTS)
                delta, dbuf = _guarded(d0)
                act = torch.full((-(-M // 16), F // 32, 64, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
                ops.dec_gemm(x0, w, ops.DEC_SWIGLU8, M, out=act, rownorm=(_ss(M, K), EPS) if norm else None, cfg=cfg,
                             wscale=s, delta=delta, delta_slot=slot, delta_slots=NSLOTS)
                y = ops.unpack_skinny(act)[:M]
                gu = _deil(d0.to(torch.bfloat16).double())
                ref = F_.silu(gu[:, :F]) * gu[:, F:]
                err = (y.double() - ref).abs()
                what = f"F={F} cfg={cfg} M={M} {enc} norm={norm} {pattern}"
                if bool(on.any()):
                    print(f"{what}: max err / |ref| {(err[on] / ref[on].abs()).max().item():.3e}")
                assert bool((err[on] <= (U8 + 2.0 ** -20) * ref[on].abs()).all()), what
                assert bool((y[~on] == 0).all()), what + ": rows without an adapter must be exact zeros"


def test_delta_refusals():
    F, K, M = 160, 512, 17
    cfg2, cfg0 = (1, 1, 7, 8), (1, 1, 8, 8)
    a = ops.pack_activation(_x(M, K))
    wp = _w(F, K, "bf16")[1]
    delta, slot = _delta(M, F), _slots("cycle", M)
    act = ops.packed_empty(M, F, torch.bfloat16, DEV)
    ws = torch.zeros(M * 2 * F, device=DEV)
    y = torch.zeros(M, 2 * F, device=DEV, dtype=torch.bfloat16)
    nat = ops.native().gemm_dec
    tail = (None, 0, -1, -1, -1, delta, slot, NSLOTS)  # row_w, f4_depth, the three switches, the delta
    # another epilogue
    with pytest.raises(ValueError, match="SwiGLU"):
        ops.dec_gemm(a, wp, 0, M, workspace=ws, cfg=cfg0, delta=delta, delta_slot=slot, delta_slots=NSLOTS)
    with pytest.raises(RuntimeError, match="epi 2"):
        nat(a, wp, None, ws, None, 1, 0, 1, 8, 8, M, None, 0.0, *tail)
    with pytest.raises(RuntimeError, match="epi 2"):
        nat(a, wp, None, None, y, 1, 1, 1, 8, 8, M, None, 0.0, *tail)
    # a grouped launch
    with pytest.raises(RuntimeError, match="grouped"):
        nat(a, wp[None].contiguous(), None, None, act[None].contiguous(), 1, 2, 1, 7, 8, M, None, 0.0, *tail)
    # the wide deferred norm: more than 16 sums per row
    wide = torch.rand(M, K // 16, device=DEV) + 1.0
    with pytest.raises(ValueError, match="16 deferred-norm"):
        ops.dec_gemm(a, wp, 2, M, out=act, rownorm=(wide, EPS), cfg=cfg2, delta=delta, delta_slot=slot, delta_slots=NSLOTS)
    with pytest.raises(RuntimeError, match="deferred-norm"):
        nat(a, wp, None, None, act, 1, 2, 1, 7, 8, M, wide, EPS, *tail)
    # a delta that is not what the kernel reads
    with pytest.raises(RuntimeError, match="delta"):
        nat(a, wp, None, None, act, 1, 2, 1, 7, 8, M, None, 0.0, None, 0, -1, -1, -1, delta.double(), slot, NSLOTS)
    with pytest.raises(RuntimeError, match="delta_slot"):
        nat(a, wp, None, None, act, 1, 2, 1, 7, 8, M, None, 0.0, None, 0, -1, -1, -1, delta, slot.long(), NSLOTS)
    # and the accepted call still runs
    assert nat(a, wp, None, None, act, 1, 2, 1, 7, 8, M, None, 0.0, *tail) == 1
