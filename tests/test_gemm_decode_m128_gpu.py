"""The shared-A decode GEMM (gemm_decode.hip) at 65..128 rows - the 5..8 m-tile instantiations -
against an fp32 reference of the same product, with the bound of tests/test_gemm_decode_gpu.py
(err <= 2.5e-2 * scale + 1e-3; 3e-2 for the deferred-norm cases).

Row counts, each the smallest at which one thing can break: 65 (first row of m-tile 5, a ragged
tile), 97 (the first row a 6-wave deferred-norm prologue of 4 threads per row does not reach in
one pass), 113 (the same for a 7-wave workgroup), 128 (full: 128.5 KiB of LDS).  Weights and their
packed copies are made once per shape and shared by the cases."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F_ = torch.nn.functional
MS = [65, 97, 113, 128]


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    _w.cache_clear()
    _wp.cache_clear()
    _w13p.cache_clear()


def _check(y, ref, what, tol=2.5e-2):
    err = (y.float() - ref.float()).abs().max().item()
    scale = ref.float().abs().max().item()
    print(f"{what}: max err {err:.4g} scale {scale:.4g}")
    assert err <= tol * scale + 1e-3, f"{what}: max err {err:.4g} vs scale {scale:.4g}"


@functools.lru_cache(maxsize=None)
def _w(N, K, seed=0):
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    return (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _wp(N, K):
    return ops.pack_skinny(_w(N, K))


@functools.lru_cache(maxsize=None)
def _w13p(F, K):
    return ops.pack_skinny(ops.interleave_gate_up8(torch.cat([_w(F, K, 1), _w(F, K, 2)])))


def _x(M, K):
    g = torch.Generator(device=DEV).manual_seed(M * 7919 + K)
    return torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)


# today's table (<= 64 rows): must not move
TODAY = {(6144, 4096, 0): (4, 1, 6, 8), (4096, 4096, 0): (8, 1, 8, 8), (28672, 4096, 2): (1, 1, 7, 8),
         (4096, 14336, 0): (8, 1, 8, 8), (128256, 4096, 1): (1, 4, 8, 4)}

CASES = [  # (N, K, cfg)
    (6144, 4096, (4, 1, 6, 8)),
    (4096, 4096, (8, 1, 8, 8)),
    (4096, 14336, (8, 1, 8, 8)),
    (1024, 512, (2, 1, 4, 8)),
    (320, 1024, (1, 1, 8, 8)),  # 20 n-tiles, 8 per workgroup: the third workgroup is ragged
]
for _N, _K in ((6144, 4096), (4096, 4096), (4096, 14336)):  # what dec_config picks above 64 rows, if different
    for _m in (65, 128):
        _c = ops.dec_config(_N, _K, 0, rows=_m)
        if (_N, _K, _c) not in CASES:
            CASES.append((_N, _K, _c))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K,cfg", CASES)
def test_dec_slabs_match_fp32_above_64_rows(M, N, K, cfg):
    x, w = _x(M, K), _w(N, K)
    S = cfg[0]
    ws = torch.full((S * M * N + 64,), float("nan"), device=DEV, dtype=torch.float32)
    s = ops.dec_gemm(ops.pack_activation(x), _wp(N, K), 0, M, workspace=ws, cfg=cfg)
    assert s == S
    assert not torch.isnan(ws[: s * M * N]).any(), "every slab element written"
    assert torch.isnan(ws[s * M * N:]).all(), "nothing written past the slabs"
    y = ws[: s * M * N].view(s, M, N).sum(0)
    _check(y, x.float() @ w.float().t(), f"slabs M{M} N{N} K{K} cfg{cfg}")
    kc = K // s  # every slab is the product over its own K slice
    last = x[:, (s - 1) * kc:].float() @ w[:, (s - 1) * kc:].float().t()
    _check(ws[(s - 1) * M * N: s * M * N].view(M, N), last, "last slab")


def _rows_scaled(M, K):
    """Residual rows with very different norms (row i scaled by 1 + i / 8): a missing or another
    row's 1/rms is off by up to 17x and cannot pass the bound."""
    return (_x(M, K).float() * (1 + torch.arange(M, device=DEV).float() / 8).unsqueeze(1)).to(torch.bfloat16)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K,cfg", [(6144, 4096, (4, 1, 6, 8)), (1024, 512, (2, 1, 4, 8))])
def test_dec_rownorm_scale_above_64_rows(M, N, K, cfg):
    """Deferred RMSNorm into slabs: A holds x * w; outputs scaled by 1/rms from add_norm_partial's
    sums.  6-wave (qkv) and 4-wave workgroups: fewer threads than 4 per row."""
    res = _rows_scaled(M, K)
    nw = (torch.rand(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) + 0.5).to(torch.bfloat16)
    w = _w(N, K)
    xw, ss = ops.add_norm_partial(res.clone(), None, 0, nw)
    ws = torch.full((cfg[0] * M * N,), float("nan"), device=DEV, dtype=torch.float32)
    s = ops.dec_gemm(xw, _wp(N, K), 0, M, workspace=ws, rownorm=(ss, 1e-5), cfg=cfg)
    y = ws[: s * M * N].view(s, M, N).sum(0)
    xn = F_.rms_norm(res.float(), (K,), nw.float(), 1e-5)
    _check(y, xn @ w.float().t(), f"rownorm M{M} N{N} cfg{cfg}", tol=3e-2)


@pytest.mark.parametrize("M", MS)
def test_dec_rownorm_gate_up_above_64_rows(M):
    """Deferred RMSNorm into the SwiGLU epilogue: gate_up (28672, 4096) on 7-wave workgroups."""
    K, F, cfg = 4096, 14336, (1, 1, 7, 8)
    res = _rows_scaled(M, K)
    nw = (torch.rand(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) + 0.5).to(torch.bfloat16)
    xw, ss = ops.add_norm_partial(res.clone(), None, 0, nw)
    act = ops.packed_empty(M, F, torch.bfloat16, DEV)
    ops.dec_gemm(xw, _w13p(F, K), 2, M, out=act, rownorm=(ss, 1e-5), cfg=cfg)
    xn = F_.rms_norm(res.float(), (K,), nw.float(), 1e-5)
    g = (xn @ _w(F, K, 1).float().t()).to(torch.bfloat16).float()
    u = (xn @ _w(F, K, 2).float().t()).to(torch.bfloat16).float()
    _check(ops.unpack_skinny(act)[:M], F_.silu(g) * u, f"rownorm gate_up M{M}", tol=3e-2)


@pytest.mark.parametrize("M", [65, 128])
def test_dec_swiglu8_feeds_down_above_64_rows(M):
    K, F = 4096, 14336
    x = _x(M, K)
    cfg = ops.dec_config(2 * F, K, 2, rows=M)
    act = ops.packed_empty(M, F, torch.bfloat16, DEV)
    ops.dec_gemm(ops.pack_activation(x), _w13p(F, K), 2, M, out=act, cfg=cfg)
    g = (x.float() @ _w(F, K, 1).float().t()).to(torch.bfloat16).float()
    u = (x.float() @ _w(F, K, 2).float().t()).to(torch.bfloat16).float()
    h = F_.silu(g) * u
    _check(ops.unpack_skinny(act)[:M], h, f"swiglu8 M{M} cfg{cfg}")
    # ... and the packed activation is the down projection's A operand as it stands
    N2 = 4096
    c2 = ops.dec_config(N2, F, 0, rows=M)
    ws = torch.full((c2[0] * M * N2,), float("nan"), device=DEV, dtype=torch.float32)
    s = ops.dec_gemm(act, _wp(N2, F), 0, M, workspace=ws)
    assert s == c2[0]
    hb = ops.unpack_skinny(act)[:M].float()
    _check(ws.view(s, M, N2).sum(0), hb @ _w(N2, F).float().t(), f"down after swiglu8 M{M} cfg{c2}")


@pytest.mark.parametrize("M", [65, 128])
def test_dec_bf16_lm_head_above_64_rows(M):
    """N = 128256 does not divide the workgroup tile: the last workgroup is ragged."""
    N, K = 128256, 4096
    x, w = _x(M, K), _w(N, K)
    cfg = ops.dec_config(N, K, 1, rows=M)
    y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.dec_gemm(ops.pack_activation(x), _wp(N, K), 1, M, out=y)
    assert not torch.isnan(y).any(), "every column of every row written (the ragged last workgroup included)"
    _check(y, x.float() @ w.float().t(), f"lm_head M{M} cfg{cfg}")


def test_dec_row_limits_kept():
    """128 rows for the dense launch; the grouped launch and the row-complete kernel keep 64."""
    K, N = 512, 1024
    x = _x(129, K)
    with pytest.raises((RuntimeError, ValueError)):
        ops.dec_gemm(ops.pack_activation(x), _wp(N, K), 0, 129,
                     workspace=torch.empty(2 * 129 * N, device=DEV, dtype=torch.float32), cfg=(2, 1, 4, 8))
    M, E, F, d = 65, 2, 1024, 512
    xe = _x(M, d)
    wg = torch.stack([_w13p(F, d)] * E)
    act = torch.empty((E, -(-M // 16), 2 * F // 64, 64, 8), device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.dec_gemm_grouped(ops.pack_activation(xe), wg, 2, M, out=act)
    wd = torch.stack([_wp(d, F)] * E)
    with pytest.raises(RuntimeError):
        ops.dec_gemm_grouped(act, wd, 0, M, workspace=torch.empty(E * M * d, device=DEV, dtype=torch.float32),
                             row_w=torch.ones(M, E, device=DEV))
    resid = _x(M, 4096)
    nw = torch.ones(4096, device=DEV, dtype=torch.bfloat16)
    assert ops.dec_gemm_rc(ops.pack_activation(_x(M, 4096)), _wp(4096, 4096), M, resid, nw, 1e-5) is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("M", [1, 17, 40, 64])
def test_dec_slabs_up_to_64_rows_repeatable(M):
    """<= 64 rows: slabs bit-identical between two launches of the same call."""
    N, K = 6144, 4096
    xp = ops.pack_activation(_x(M, K))
    out = []
    for _ in range(2):
        ws = torch.full((4 * M * N,), float("nan"), device=DEV, dtype=torch.float32)
        assert ops.dec_gemm(xp, _wp(N, K), 0, M, workspace=ws) == 4
        out.append(ws)
    assert torch.equal(out[0], out[1])


def test_dec_config_up_to_64_rows_unchanged():
    for (N, K, epi), cfg in TODAY.items():
        assert ops.dec_config(N, K, epi) == cfg
        for rows in (1, 33, 64):
            assert ops.dec_config(N, K, epi, rows=rows) == cfg
    assert ops.DEC_MAX_M == 128 and ops.SKINNY_MAX_M == 64
