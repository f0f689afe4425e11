"""The mxfp4-W form of the 256 x 256 prefill GEMM (ops/csrc/gemm_tile.hip, F4): W as e2m1 codes and
e8m0 block scales in the decode GEMMs' packed layout (ops.pack_skinny_f4) - the tensors decode streams.

Weights: randn * 0.02, row r times 2^(r % 7 - 3) and block b of 32 along K times 2^(b % 3 - 2), so
neighbouring rows and neighbouring blocks carry different scales (a scale taken from the wrong
k-step or row cannot pass), one all-zero row and one all-zero block, quantised with
ops.quantize_mxfp4; x is randn bf16.  Per launch, over NaN-filled outputs:
  1. torch.equal with the EXISTING bf16 packed-W launch (ops.gemm_tile / gemm_tile_resid over
     pack_skinny(dequantised), same epilogue, algo=1) - the codes convert to exactly the bf16
     weight and the MFMA sequence and epilogues are the same;
  2. the bound of tests/test_gemm_tile_gpu.py (atol 3e-2, rtol 2e-2) against the fp32 product over
     the dequantised weights (the CPU form of the same op; the magnitudes do not exceed those of
     tests/test_gemm_tile_f8_gpu.py);
  3. no NaN left where a store is due.
Shapes: K 256 (four k-tiles: one steady iteration plus the peeled tail), 384 (an odd number of
128-groups), 640 (one full period of ring slot x k-tile parity), 1408 (more than two); M 1, 255, 257,
513; N 16, 240, 272, 1296 (ragged last n-tile), 256, and workgroup counts odd for the XCD remap."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
MS = (1, 255, 257, 513)
# (K, row scale).  The row scale's launcher takes partial-sum counts that are multiples of 4: 4 and 8
# partials (K 512, 1024); the other two K run the epilogue without it.
RS_CASES = [(384, False), (640, False), (512, True), (1024, True)]
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
    """(dequantised bf16 [N, K], packed codes, packed block scales) of a row-major weight, in its row order."""
    q, s = ops.quantize_mxfp4(w)
    return (ops.dequantize_mxfp4(q, s),) + ops.pack_skinny_f4(q, s)


@functools.lru_cache(maxsize=None)
def _w(N, K, seed=0):
    g = torch.Generator(device=DEV).manual_seed(4000 + seed)
    w = torch.randn(N, K, device=DEV, generator=g) * 0.02
    w = w * torch.exp2((torch.arange(N, device=DEV) % 7 - 3).float())[:, None]
    w = w * torch.exp2((torch.arange(K // 32, device=DEV) % 3 - 2).float()).repeat_interleave(32)[None, :]
    w[N // 3] = 0  # an all-zero row: every block scale 2^0, every code 0
    w[(2 * N) // 3, 32 * (K // 64):32 * (K // 64) + 32] = 0  # and one all-zero block of another row
    return _quant(w.to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def _w13(F, K):
    """[8 gate | 8 up] interleaved rows of F gate and F up features from different draws:
    dequantised interleaved weight, packed codes, packed block scales."""
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
    """mxfp4 launch on a NaN-filled output == bf16 packed launch, both within the bound of the fp32
    CPU form; returns the mxfp4 result."""
    cpu = {k: (tuple(t.cpu() if torch.is_tensor(t) else t for t in v) if isinstance(v, tuple) else v)
           for k, v in kw.items()}
    r32 = ops.gemm_tile(x.cpu(), dq.cpu(), algo=1, **cpu)
    out = torch.full(r32.shape, NAN, device=DEV, dtype=torch.bfloat16)
    y4 = ops.gemm_tile(x, qp, algo=1, out=out, wscale=s, **kw)
    yb = ops.gemm_tile(x, ops.pack_skinny(dq), algo=1, **kw)
    assert not torch.isnan(y4).any(), f"{what}: a due store is missing"
    assert torch.equal(y4, yb), f"{what}: mxfp4 W differs from the bf16 packed launch"
    _close(y4.cpu(), r32, what)
    return y4


@pytest.mark.parametrize("K", [256, 384, 640, 1408])
@pytest.mark.parametrize("N", [16, 240, 256, 272, 1296])
def test_tile_f4_plain(N, K):
    dq, qp, s = _w(N, K)
    for M in MS:
        _three(_x(M, K), dq, qp, s, f"plain {M}x{N}x{K}")


@pytest.mark.parametrize("K,rs", RS_CASES)
def test_tile_f4_rope(K, rs):
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
def test_tile_f4_swiglu8(N, K, rs):
    il, qp, s = _w13(N // 2, K)
    for M in (1, 255, 513):
        kw = dict(swiglu=8)
        if rs:
            kw["rowscale"] = (_ss(M, K), 1e-5)
        _three(_x(M, K), il, qp, s, f"swiglu8 {M}x{N}x{K} rs={rs}", **kw)


@pytest.mark.parametrize("N,K", [(128, 512), (384, 768), (1280, 256)])
def test_tile_f4_resid(N, K):
    dq, qp, s = _w(N, K)
    for M in MS:
        x = _x(M, K)
        g = torch.Generator(device=DEV).manual_seed(N + M)
        resid = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
        nw = (torch.rand(N, device=DEV, generator=g) + 0.5).to(torch.bfloat16)
        r4, rb, rc = resid.clone(), resid.clone(), resid.cpu().clone()
        hw = torch.full((M, N), NAN, device=DEV, dtype=torch.bfloat16)
        ss = torch.full((M, N // 128), NAN, device=DEV, dtype=torch.float32)
        h4, s4 = ops.gemm_tile_resid(x, qp, r4, nw, hw=hw, ss=ss, wscale=s)
        hb, sb = ops.gemm_tile_resid(x, ops.pack_skinny(dq), rb, nw)
        hc, sc = ops.gemm_tile_resid(x.cpu(), dq.cpu(), rc, nw.cpu())
        what = f"resid {M}x{N}x{K}"
        assert not (torch.isnan(r4).any() or torch.isnan(h4).any() or torch.isnan(s4).any()), what
        assert torch.equal(r4, rb) and torch.equal(h4, hb) and torch.equal(s4, sb), what
        _close(r4.cpu(), rc, what + " resid")
        _close(h4.cpu(), hc, what + " hw")
        _close(s4.cpu(), sc, what + " ss")


def test_tile_f4_asymmetric_identity():
    """A = I with W[n, k] = grid[(3n + 7k) % 15] * 2^((k // 32) % 3 - 1) over the fifteen distinct
    e2m1 values: a swapped nibble, byte, sub-step, k-tile parity or scale byte cannot pass."""
    K = 256
    x = torch.eye(256, K, device=DEV, dtype=torch.bfloat16)
    grid = torch.tensor([-6, -4, -3, -2, -1.5, -1, -0.5, 0, 0.5, 1, 1.5, 2, 3, 4, 6], device=DEV)
    n = torch.arange(256, device=DEV)[:, None]
    k = torch.arange(K, device=DEV)[None, :]
    w = (grid[(3 * n + 7 * k) % 15] * torch.exp2(((k // 32) % 3 - 1).float())).to(torch.bfloat16)
    dq, qp, s = _quant(w)
    assert torch.equal(dq, w), "the e2m1 grid times a power of two dequantises to itself"
    y = ops.gemm_tile(x, qp, algo=1, wscale=s)
    assert torch.equal(y.float().cpu(), w.float().t().cpu())


def test_tile_f4_unsupported_forms_raise():
    """Grouped launches, K = 128, algo=0, the per-128 SwiGLU pairing and missing or mis-shaped scales
    have no mxfp4 form: an error, never another path."""
    dq, qp, s = _w(256, 256)
    x = _x(64, 256)
    off = torch.tensor([0, 64], dtype=torch.int32, device=DEV)
    _, qp128, s128 = _quant((torch.randn(256, 128, device=DEV) * 0.02).to(torch.bfloat16))
    with pytest.raises((ValueError, RuntimeError), match="schedule"):
        ops.gemm_tile(x, qp, algo=0, wscale=s)
    with pytest.raises((ValueError, RuntimeError), match="grouped"):
        ops.gemm_tile(x, qp[None].contiguous(), off, algo=1, wscale=s)
    with pytest.raises((ValueError, RuntimeError), match="swiglu"):
        ops.gemm_tile(x, qp, swiglu=True, algo=1, wscale=s)
    with pytest.raises((ValueError, RuntimeError), match="scale"):
        ops.gemm_tile(x, qp, algo=1)
    with pytest.raises((ValueError, RuntimeError), match="scale"):
        ops.gemm_tile(x, qp, algo=1, wscale=s.reshape(16, 2, 64))
    with pytest.raises((ValueError, RuntimeError), match="scale"):
        ops.gemm_tile(x, qp, algo=1, wscale=s.float())
    with pytest.raises((ValueError, RuntimeError), match="K"):
        ops.gemm_tile(_x(64, 128), qp128, algo=1, wscale=s128)
    # the extension refuses them too (no fall-back below the Python checks)
    y = torch.empty(64, 256, device=DEV, dtype=torch.bfloat16)
    gt = ops.native().gemm_tile
    with pytest.raises(RuntimeError):
        gt(y, x, qp, None, 0, 0, wscale=s)  # schedule 0
    with pytest.raises(RuntimeError):
        gt(torch.empty(64, 128, device=DEV, dtype=torch.bfloat16), x, qp, None, 1, 1, wscale=s)  # per-128 SwiGLU
    with pytest.raises(RuntimeError):
        gt(y, x, qp[None].contiguous(), off, 0, 1, wscale=s)  # grouped
    with pytest.raises(RuntimeError):
        gt(y, _x(64, 128), qp128, None, 0, 1, wscale=s128)  # K = 128
    with pytest.raises(RuntimeError):
        gt(y, x, qp, None, 0, 1)  # no scales
    with pytest.raises(RuntimeError):
        gt(y, x, qp, None, 0, 1, wscale=s.reshape(16, 2, 64))
    with pytest.raises(RuntimeError):
        gt(y, x, qp, None, 0, 1, wscale=s.float())
