"""Every compiled form of the shared-A decode GEMM (ops.DEC_FORMS, the table gemm_decode.hip
dispatches from) launched once per row class against an fp32 product, with the bounds of
tests/test_gemm_decode_gpu.py (err <= 2.5e-2 * scale + 1e-3; 3e-2 with a deferred norm).  Driven
by the table: a form added to it is covered without an edit here.

Per form: rows 1, 16 * min(max m-tiles, 4) and, above 4 m-tiles, 65 and 16 * max m-tiles; K = 512
(two A chunks, one or two turns of the weight ring); splits 1, and 2 for the SLAB forms of depth 8;
N one n-tile past two full workgroups (SLAB, BF16) or four n-tiles past four (SWIGLU8), so the last
workgroup is ragged.  Wide-norm forms once more at 1 and 64 rows over per-16-column sums."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F_ = torch.nn.functional
K = 512


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    _w.cache_clear()


def _check(y, ref, what, tol=2.5e-2):
    err = (y.float() - ref.float()).abs().max().item()
    scale = ref.float().abs().max().item()
    print(f"{what}: max err {err:.4g} scale {scale:.4g}")
    assert err <= tol * scale + 1e-3, f"{what}: max err {err:.4g} vs scale {scale:.4g}"


@functools.lru_cache(maxsize=None)
def _w(N, seed=0):
    g = torch.Generator(device=DEV).manual_seed(2000 + seed)
    return (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(torch.bfloat16)


def _x(M):
    g = torch.Generator(device=DEV).manual_seed(M * 7919 + K)
    return torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)


def _launch(epi, cfg, N, M, a, rownorm=None):
    """One dec_gemm launch over NaN-filled outputs; returns the [M, N] (SWIGLU8: [M, N / 2]) result."""
    S = cfg[0]
    if epi == ops.DEC_SLAB:
        ws = torch.full((S * M * N + 64,), float("nan"), device=DEV, dtype=torch.float32)
        assert ops.dec_gemm(a, ops.pack_skinny(_w(N)), epi, M, workspace=ws, rownorm=rownorm, cfg=cfg) == S
        assert not torch.isnan(ws[: S * M * N]).any(), "every slab element written"
        assert torch.isnan(ws[S * M * N:]).all(), "nothing written past the slabs"
        return ws[: S * M * N].view(S, M, N).sum(0)
    if epi == ops.DEC_BF16:
        y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        ops.dec_gemm(a, ops.pack_skinny(_w(N)), epi, M, out=y, rownorm=rownorm, cfg=cfg)
        assert not torch.isnan(y).any(), "every column of every row written (the ragged last workgroup included)"
        return y
    F = N // 2
    w13 = ops.pack_skinny(ops.interleave_gate_up8(torch.cat([_w(F, 1), _w(F, 2)])))
    act = torch.full((-(-M // 16), F // 32, 64, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.dec_gemm(a, w13, epi, M, out=act, rownorm=rownorm, cfg=cfg)
    y = ops.unpack_skinny(act)[:M]
    assert not torch.isnan(y).any(), "every feature of every row written"
    return y


def _ref(epi, N, xf):
    """The fp32 product of rows xf [M, K] (SWIGLU8: gate and up rounded to bf16 first, as the kernel)."""
    if epi != ops.DEC_SWIGLU8:
        return xf @ _w(N).float().t()
    g = (xf @ _w(N // 2, 1).float().t()).to(torch.bfloat16).float()
    u = (xf @ _w(N // 2, 2).float().t()).to(torch.bfloat16).float()
    return F_.silu(g) * u


@pytest.mark.parametrize("form", ops.DEC_FORMS, ids=lambda f: "epi{}-ntw{}-w{}-d{}-mt{}-wide{}".format(*f))
def test_dec_form_matches_fp32(form):
    epi, ntw, waves, depth, max_mt, wide = form
    N = 64 * (waves + 1) if epi == ops.DEC_SWIGLU8 else 16 * (2 * ntw * waves + 1)
    rows = [1, 16 * min(max_mt, 4)] + ([65, 16 * max_mt] if max_mt > 4 else [])
    splits = [1, 2] if epi == ops.DEC_SLAB and depth == 8 else [1]
    for M in rows:
        x = _x(M)
        ref = _ref(epi, N, x.float())
        for S in splits:
            cfg = (S, ntw, waves, depth)
            _check(_launch(epi, cfg, N, M, ops.pack_activation(x)), ref, f"{form} M{M} S{S}")
    if wide:  # the deferred RMSNorm over per-16-column sums of squares (what dec_gemm_rc leaves)
        nw = (torch.rand(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) + 0.5).to(torch.bfloat16)
        for M in (1, 64):
            # rows of very different norms: another row's 1/rms cannot pass the bound
            res = (_x(M).float() * (1 + torch.arange(M, device=DEV).float() / 8).unsqueeze(1)).to(torch.bfloat16)
            ss = (res.float() ** 2).view(M, K // 16, 16).sum(-1).contiguous()
            xw = ops.pack_activation((res.float() * nw.float()).to(torch.bfloat16))
            y = _launch(epi, (1, ntw, waves, depth), N, M, xw, rownorm=(ss, 1e-5))
            xn = F_.rms_norm(res.float(), (K,), nw.float(), 1e-5)
            _check(y, _ref(epi, N, xn), f"{form} wide norm M{M}", tol=3e-2)
    if max_mt == 4:  # no 5 m-tile instantiation: refused by the table, before any launch
        with pytest.raises(RuntimeError, match="not compiled for 65 rows"):
            _launch(epi, (1, ntw, waves, depth), N, 65, ops.pack_activation(_x(65)))
    torch.cuda.synchronize()
