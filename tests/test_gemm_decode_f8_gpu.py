"""The fp8-weight instantiations of the shared-A decode GEMM (ops.DEC_F8_FORMS), with the shapes of
tests/test_gemm_decode_forms_gpu.py: K = 512; rows 1, 16 * min(max m-tiles, 4) and, above 4
m-tiles, 65 and 16 * max m-tiles; N ragged in the last workgroup; splits 1, and 2 for the SLAB
forms of depth 8; NaN-filled outputs.

Weight row r is multiplied by 2^(r % 7 - 3) before quantising, so neighbouring rows carry
different scales: a scale read in canonical instead of packed order, or a gate / up mix-up, cannot
pass.  Per launch:
  1. bit equality (torch.equal) with the bf16 dec_gemm of the same configuration over
     pack_skinny(dequantised weights) - SLAB slab by slab: the codes convert to bf16 exactly, the
     MFMA sequence is the same, and the power-of-two scale on the fp32 accumulator commutes with
     every rounding;
  2. the project's bound against the fp32 product over the dequantised weights
     (2.5e-2 * scale + 1e-3; 3e-2 with the deferred norm)."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F_ = torch.nn.functional
K = 512
F8_FORMS = [ops.DEC_FORMS[i] for i in ops.DEC_F8_FORMS]
_ID = "epi{}-ntw{}-w{}-d{}-mt{}-wide{}"


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    _w.cache_clear()
    _w13.cache_clear()


def _check(y, ref, what, tol=2.5e-2):
    err = (y.float() - ref.float()).abs().max().item()
    scale = ref.float().abs().max().item()
    print(f"{what}: max err {err:.4g} scale {scale:.4g}")
    assert err <= tol * scale + 1e-3, f"{what}: max err {err:.4g} vs scale {scale:.4g}"


def _quant(w):
    """(dequantised bf16 [N, K], packed codes, scales) of a row-major weight in its packed row order."""
    q, s = ops.quantize_rows_fp8(w)
    return ops.dequantize_rows_fp8(q, s), ops.pack_skinny_f8(q), s


@functools.lru_cache(maxsize=None)
def _w(N, seed=0):
    g = torch.Generator(device=DEV).manual_seed(2000 + seed)
    w = torch.randn(N, K, device=DEV, generator=g) * 0.02
    w = w * torch.exp2((torch.arange(N, device=DEV) % 7 - 3).float())[:, None]  # visibly different row scales
    return _quant(w.to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def _w13(F):
    """gate / up weights of F features each: the dequantised [gate; up], and the packed encodings of
    the [8 gate | 8 up] interleaved rows (the scales permuted with them)."""
    gu = torch.cat([_w(F, 1)[0], _w(2 * F, 2)[0][F:]])  # up rows F.. of another draw: other scales than gate's
    il = ops.interleave_gate_up8(gu)
    dq, qp, s = _quant(il)
    assert torch.equal(dq, il), "dequantised values are stable under re-quantisation"
    return gu, ops.pack_skinny(il), qp, s


def _x(M):
    g = torch.Generator(device=DEV).manual_seed(M * 7919 + K)
    return torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)


def _launch(epi, cfg, N, M, a, f8, rownorm=None):
    """One dec_gemm launch over NaN-filled outputs, over the fp8 (``f8``) or the bf16 encoding of the
    same weights; returns the raw output: SLAB [S, M, N] fp32, BF16 [M, N], SWIGLU8 [M, N / 2]."""
    S = cfg[0]
    if epi == ops.DEC_SWIGLU8:
        _, wp, qp, s = _w13(N // 2)
    else:
        dq, qp, s = _w(N)
        wp = ops.pack_skinny(dq)
    kw = dict(wscale=s) if f8 else {}
    w = qp if f8 else wp
    if epi == ops.DEC_SLAB:
        ws = torch.full((S * M * N + 64,), float("nan"), device=DEV, dtype=torch.float32)
        assert ops.dec_gemm(a, w, epi, M, workspace=ws, rownorm=rownorm, cfg=cfg, **kw) == S
        assert not torch.isnan(ws[: S * M * N]).any(), "every slab element written"
        assert torch.isnan(ws[S * M * N:]).all(), "nothing written past the slabs"
        return ws[: S * M * N].view(S, M, N)
    if epi == ops.DEC_BF16:
        y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        ops.dec_gemm(a, w, epi, M, out=y, rownorm=rownorm, cfg=cfg, **kw)
        assert not torch.isnan(y).any(), "every column of every row written (the ragged last workgroup included)"
        return y
    act = torch.full((-(-M // 16), N // 64, 64, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.dec_gemm(a, w, epi, M, out=act, rownorm=rownorm, cfg=cfg, **kw)
    y = ops.unpack_skinny(act)[:M]
    assert not torch.isnan(y).any(), "every feature of every row written"
    return y


def _ref(epi, N, xf):
    """The fp32 product of rows xf [M, K] over the dequantised weights (SWIGLU8: gate and up rounded
    to bf16 first, as the kernel)."""
    if epi != ops.DEC_SWIGLU8:
        return xf @ _w(N)[0].float().t()
    gu = _w13(N // 2)[0].float()
    g = (xf @ gu[: N // 2].t()).to(torch.bfloat16).float()
    u = (xf @ gu[N // 2:].t()).to(torch.bfloat16).float()
    return F_.silu(g) * u


def _both(epi, cfg, N, M, a, ref, what, rownorm=None, tol=2.5e-2):
    y8 = _launch(epi, cfg, N, M, a, True, rownorm)
    yb = _launch(epi, cfg, N, M, a, False, rownorm)
    same = torch.equal(y8, yb)
    diff = (y8.float() - yb.float()).abs().max().item()
    print(f"{what}: fp8 vs bf16 launch bit-equal {same}, max diff {diff:.4g}")
    assert same, f"{what}: the fp8 launch differs from the bf16 launch over the dequantised weights (max {diff:.4g})"
    _check(y8.sum(0) if epi == ops.DEC_SLAB else y8, ref, what, tol)


def _shape_n(epi, ntw, waves):
    return 64 * (waves + 1) if epi == ops.DEC_SWIGLU8 else 16 * (2 * ntw * waves + 1)


@pytest.mark.parametrize("form", F8_FORMS, ids=lambda f: _ID.format(*f))
def test_f8_form_bit_equal_to_bf16_and_within_bound(form):
    epi, ntw, waves, depth, max_mt, _ = form
    N = _shape_n(epi, ntw, waves)
    rows = [1, 16 * min(max_mt, 4)] + ([65, 16 * max_mt] if max_mt > 4 else [])
    splits = [1, 2] if epi == ops.DEC_SLAB and depth == 8 else [1]
    for M in rows:
        x = _x(M)
        ref = _ref(epi, N, x.float())
        for S in splits:
            _both(epi, (S, ntw, waves, depth), N, M, ops.pack_activation(x), ref, f"{form} M{M} S{S}")
    if max_mt == 4:  # no 5 m-tile instantiation: refused by the table, before any launch
        with pytest.raises(RuntimeError, match="not compiled for 65 rows over fp8 weights"):
            _launch(epi, (1, ntw, waves, depth), N, 65, ops.pack_activation(_x(65)), True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", F8_FORMS, ids=lambda f: _ID.format(*f))
def test_f8_form_narrow_deferred_norm(form):
    """The deferred RMSNorm over per-512-column sums of squares (what add_norm_partial leaves), rows
    of very different norms: another row's 1/rms cannot pass the bound."""
    epi, ntw, waves, depth, max_mt, _ = form
    N = _shape_n(epi, ntw, waves)
    nw = (torch.rand(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) + 0.5).to(torch.bfloat16)
    for M in [m for m in (1, 64, 128) if m <= 16 * max_mt]:
        res = (_x(M).float() * (1 + torch.arange(M, device=DEV).float() / 8).unsqueeze(1)).to(torch.bfloat16)
        ss = (res.float() ** 2).view(M, K // 512, 512).sum(-1).contiguous()
        xw = ops.pack_activation((res.float() * nw.float()).to(torch.bfloat16))
        xn = F_.rms_norm(res.float(), (K,), nw.float(), 1e-5)
        _both(epi, (1, ntw, waves, depth), N, M, xw, _ref(epi, N, xn), f"{form} narrow norm M{M}",
              rownorm=(ss, 1e-5), tol=3e-2)
    torch.cuda.synchronize()


def test_every_finite_e4m3_code_converts_exactly():
    """Weight rows hold all 254 finite codes at scale 1; one-hot activation rows select the k
    positions; the BF16 epilogue must return each value exactly."""
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8, device=DEV)
    assert codes.numel() == 254
    epi, ntw, waves, depth = next(f for f in F8_FORMS if f[0] == ops.DEC_BF16)[:4]
    N, M = 16 * ntw * waves, 64
    # row n, column k holds code (n * 37 + k * 11) % 254: every code in every row, at varying k % 64
    idx = (torch.arange(N, device=DEV)[:, None] * 37 + torch.arange(K, device=DEV)[None, :] * 11) % 254
    q = codes[idx].view(torch.float8_e4m3fn)
    vals = q.float()
    assert torch.isfinite(vals).all() and vals.unique().numel() == 253  # +0 and -0 compare equal
    qp, s = ops.pack_skinny_f8(q), torch.ones(N, device=DEV)
    for base in range(0, K, M):  # one-hot rows over every k position
        x = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
        x[torch.arange(M), base + torch.arange(M)] = 1
        y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        ops.dec_gemm(ops.pack_activation(x), qp, epi, M, out=y, cfg=(1, ntw, waves, depth), wscale=s)
        want = vals[:, base:base + M].t().to(torch.bfloat16)
        assert torch.equal(y, want), f"k {base}..{base + M - 1}: a code converted inexactly or out of place"
    torch.cuda.synchronize()


def test_form_without_fp8_instantiation_raises_before_launch():
    out_forms = [f for i, f in enumerate(ops.DEC_FORMS) if i not in ops.DEC_F8_FORMS]
    assert out_forms, "some form stays bf16-only"
    for epi, ntw, waves, depth, _, _ in out_forms:
        N = _shape_n(epi, ntw, waves)
        with pytest.raises(RuntimeError, match="over fp8 weights"):
            _launch(epi, (1, ntw, waves, depth), N, 1, ops.pack_activation(_x(1)), True)
    torch.cuda.synchronize()
