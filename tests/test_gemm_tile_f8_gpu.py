"""The fp8-W form of the 256 x 256 prefill GEMM (ops/csrc/gemm_tile.hip, F8): W as e4m3 codes in the
decode GEMMs' packed layout (ops.pack_skinny_f8) with per-row power-of-two scales.

Weights as in tests/test_gemm_decode_f8_gpu.py: randn * 0.02, row r times 2^(r % 7 - 3) so that
neighbouring rows carry different scales, one all-zero row, quantised with ops.quantize_rows_fp8;
x is randn bf16.  Every code * 2^e and every product is then a normal number.  Per launch, over
NaN-filled outputs:
  1. torch.equal with the EXISTING bf16 packed-W launch (ops.gemm_tile / gemm_tile_resid over
     pack_skinny(dequantised), same epilogue, algo=1) - the codes convert to exactly the bf16
     weight and the MFMA sequence and epilogues are the same;
  2. the bound of tests/test_gemm_tile_gpu.py (atol 3e-2, rtol 2e-2) against the fp32 product over
     the dequantised weights (the CPU form of the same op);
  3. no NaN left where a store is due.
Shapes: K 192 (the peeled ring tail only), 256 (one steady iteration), 320 (odd tile count), 704
(more than one 5-slot ring period); M 1, 255, 257, 513; N 16, 240, 272, 1296 (ragged last n-tile),
256, and workgroup counts that are odd for the XCD remap."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
MS = (1, 255, 257, 513)
# (K, row scale).  The row scale reads its K / 128 partial sums four at a time, so the launcher
# takes multiples of 4 only (4 is the smallest): 4 and 8 partials here, and K = 768 (6 partials)
# runs without the row scale and must be refused with it, as the bf16 form refuses it.
RS_CASES = [(320, False), (768, False), (512, True), (1024, True)]
NAN = float("nan")


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    for f in (_w, _w13, _x, _cs):
        f.cache_clear()


def _close(a, b, what, atol=3e-2, rtol=2e-2):
    err = (a.float() - b.float()).abs()
    tol = atol + rtol * b.float().abs()
    bad = (err > tol).sum().item()
    print(f"{what}: max err {err.max().item():.4g}")
    assert bad == 0, f"{what}: {bad} elements out of tolerance, max err {err.max().item():.4g}"


def _quant(w):
    """(dequantised bf16 [N, K], packed codes, scales) of a row-major weight, in its row order."""
    q, s = ops.quantize_rows_fp8(w)
    return ops.dequantize_rows_fp8(q, s), ops.pack_skinny_f8(q), s


@functools.lru_cache(maxsize=None)
def _w(N, K, seed=0):
    g = torch.Generator(device=DEV).manual_seed(3000 + seed)
    w = torch.randn(N, K, device=DEV, generator=g) * 0.02
    w = w * torch.exp2((torch.arange(N, device=DEV) % 7 - 3).float())[:, None]
    w[N // 3] = 0  # an all-zero row: scale 2^0, every code 0
    return _quant(w.to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def _w13(F, K):
    """[8 gate | 8 up] interleaved rows of F gate and F up features whose scales differ (the up rows
    come from another draw): dequantised interleaved weight, packed codes, permuted scales."""
    gu = torch.cat([_w(F, K, 1)[0], _w(2 * F, K, 2)[0][F:]])
    il = ops.interleave_gate_up8(gu).contiguous()
    dq, qp, s = _quant(il)
    assert torch.equal(dq, il), "dequantised values are stable under re-quantisation"
    return il, qp, s


@functools.lru_cache(maxsize=None)
def _x(M, K):
    g = torch.Generator(device=DEV).manual_seed(M * 7919 + K)
    return torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _cs():
    return ref.rope_cos_sin(4096, 128, 500000.0).to(DEV).float().contiguous()


def _ss(M, K):
    g = torch.Generator(device=DEV).manual_seed(M + K)
    return (torch.rand(M, K // 128, device=DEV, generator=g) * 64 + 16).contiguous()


def _three(x, dq, qp, s, what, **kw):
    """fp8 launch on a NaN-filled output == bf16 packed launch, both within the bound of the fp32
    CPU form; returns the fp8 result."""
    cpu = {k: (tuple(t.cpu() if torch.is_tensor(t) else t for t in v) if isinstance(v, tuple) else v)
           for k, v in kw.items()}
    r32 = ops.gemm_tile(x.cpu(), dq.cpu(), algo=1, **cpu)
    out = torch.full(r32.shape, NAN, device=DEV, dtype=torch.bfloat16)
    y8 = ops.gemm_tile(x, qp, algo=1, out=out, wscale=s, **kw)
    yb = ops.gemm_tile(x, ops.pack_skinny(dq), algo=1, **kw)
    assert not torch.isnan(y8).any(), f"{what}: a due store is missing"
    assert torch.equal(y8, yb), f"{what}: fp8 W differs from the bf16 packed launch"
    _close(y8.cpu(), r32, what)
    return y8


@pytest.mark.parametrize("K", [192, 256, 320, 704])
@pytest.mark.parametrize("N", [16, 240, 256, 272, 1296])
def test_tile_f8_plain(N, K):
    dq, qp, s = _w(N, K)
    for M in MS:
        _three(_x(M, K), dq, qp, s, f"plain {M}x{N}x{K}")


@pytest.mark.parametrize("K,rs", RS_CASES)
def test_tile_f8_rope(K, rs):
    """N = 384: three heads, two rotated; positions out of order; row scale with 4 and 8 partials."""
    N = 384
    dq, qp, s = _w(N, K)
    for M in (1, 257, 513):
        pos = ((torch.arange(M, device=DEV) * 37 + 11) % 4096).to(torch.int32)
        kw = dict(rope=(pos, _cs(), 2))
        if rs:
            kw["rowscale"] = (_ss(M, K), 1e-5)
        _three(_x(M, K), dq, qp, s, f"rope {M}x{N}x{K} rs={rs}", **kw)


@pytest.mark.parametrize("K,rs", RS_CASES)
@pytest.mark.parametrize("N", [512, 768])
def test_tile_f8_swiglu8(N, K, rs):
    il, qp, s = _w13(N // 2, K)
    for M in (1, 255, 513):
        kw = dict(swiglu=8)
        if rs:
            kw["rowscale"] = (_ss(M, K), 1e-5)
        _three(_x(M, K), il, qp, s, f"swiglu8 {M}x{N}x{K} rs={rs}", **kw)


@pytest.mark.parametrize("N,K", [(128, 512), (384, 768), (1280, 256)])
def test_tile_f8_resid(N, K):
    dq, qp, s = _w(N, K)
    for M in MS:
        x = _x(M, K)
        g = torch.Generator(device=DEV).manual_seed(N + M)
        resid = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
        nw = (torch.rand(N, device=DEV, generator=g) + 0.5).to(torch.bfloat16)
        r8, rb, rc = resid.clone(), resid.clone(), resid.cpu().clone()
        hw = torch.full((M, N), NAN, device=DEV, dtype=torch.bfloat16)
        ss = torch.full((M, N // 128), NAN, device=DEV, dtype=torch.float32)
        h8, s8 = ops.gemm_tile_resid(x, qp, r8, nw, hw=hw, ss=ss, wscale=s)
        hb, sb = ops.gemm_tile_resid(x, ops.pack_skinny(dq), rb, nw)
        hc, sc = ops.gemm_tile_resid(x.cpu(), dq.cpu(), rc, nw.cpu())
        what = f"resid {M}x{N}x{K}"
        assert not (torch.isnan(r8).any() or torch.isnan(h8).any() or torch.isnan(s8).any()), what
        assert torch.equal(r8, rb) and torch.equal(h8, hb) and torch.equal(s8, sb), what
        _close(r8.cpu(), rc, what + " resid")
        _close(h8.cpu(), hc, what + " hw")
        _close(s8.cpu(), sc, what + " ss")


def test_tile_f8_asymmetric_identity():
    """A = I with an asymmetric W of small integers (exact in e4m3): a transposed fragment or a
    swapped pair of k sub-steps cannot pass."""
    K = 256
    x = torch.eye(256, K, device=DEV, dtype=torch.bfloat16)
    n = torch.arange(512, device=DEV).float()[:, None]
    k = torch.arange(K, device=DEV).float()[None, :]
    w = ((n * 3 + k * 7) % 15 - 7).to(torch.bfloat16)
    dq, qp, s = _quant(w)
    assert torch.equal(dq, w), "small integers are exact in e4m3"
    y = ops.gemm_tile(x, qp, algo=1, wscale=s)
    assert torch.equal(y.float().cpu(), w.float().t().cpu()[:256])


def test_tile_f8_unsupported_forms_raise():
    """Grouped launches, K = 128 (schedule 0 territory), algo=0 and the per-128 SwiGLU pairing have
    no fp8 form: an error, never another path."""
    dq, qp, s = _w(256, 256)
    x = _x(64, 256)
    with pytest.raises((ValueError, RuntimeError), match="schedule"):
        ops.gemm_tile(x, qp, algo=0, wscale=s)
    with pytest.raises((ValueError, RuntimeError), match="grouped"):
        off = torch.tensor([0, 64], dtype=torch.int32, device=DEV)
        ops.gemm_tile(x, qp[None].contiguous(), off, algo=1, wscale=s)
    with pytest.raises((ValueError, RuntimeError), match="swiglu"):
        ops.gemm_tile(x, qp, swiglu=True, algo=1, wscale=s)
    with pytest.raises((ValueError, RuntimeError), match="scale"):
        ops.gemm_tile(x, qp, algo=1)
    _, qp128, s128 = _quant((torch.randn(256, 128, device=DEV) * 0.02).to(torch.bfloat16))
    with pytest.raises((ValueError, RuntimeError), match="K"):
        ops.gemm_tile(_x(64, 128), qp128, algo=1, wscale=s128)
    dq6, qp6, s6 = _w(384, 768)
    for w, kw in ((qp6, dict(wscale=s6)), (ops.pack_skinny(dq6), {})):  # 6 partial sums: no form, fp8 or bf16
        with pytest.raises((ValueError, RuntimeError)):
            ops.gemm_tile(_x(257, 768), w, swiglu=8, algo=1, rowscale=(_ss(257, 768), 1e-5), **kw)
    # the extension refuses them too (no fall-back below the Python checks)
    y = torch.empty(64, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.native().gemm_tile(y, x, qp, None, 0, 0, wscale=s)
    with pytest.raises(RuntimeError):
        ops.native().gemm_tile(y, _x(64, 128), qp128, None, 0, 1, wscale=s128)
