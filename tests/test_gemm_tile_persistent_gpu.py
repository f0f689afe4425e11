"""The persistent form of the prefill tile GEMM (gemm_tile.hip PERSIST) against the one-tile form of
the same launch, BITWISE: each output element sees the same MFMA sequence and the same epilogue
arithmetic, whichever workgroup computes its tile.

The launches are the fused-norm prefill layer's: qkv (RoPE + row scale), o and down (residual add +
the next norm's operands: resid, hw and ss_out are all compared), gate_up (SwiGLU8 + row scale),
over M in {512, 700 (a ragged last m-tile)} x N in {512, 768} x K in {192 (three k-tiles, the least
schedule 1 takes), 256, 4096}.  The row scale needs K / 128 partial sums per row in fours (tile_plan),
so K = 192 and 256 exist for the residual kind only; the row-scaled kinds take K = 512, their least,
in their place.  down's own depth (K = 14336) is one more residual case.

The A/B constants force the persistent form onto a grid of 3 workgroups (ops.TILE_PERSIST = 1,
ops.TILE_PERSIST_CUS = 3): the 4, 6 or 9 tiles of these shapes then give workgroups that cross one
or two seams, workgroups with one tile, and odd and even tile counts.  A guard row of NaNs behind
every output must stay untouched.  One launch is also checked against F.linear in fp32 at the
tolerance of tests/test_gemm_tile_gpu.py."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
ROPE, RESID, SWIGLU8 = ops.TILE_EPI_ROPE, ops.TILE_EPI_RESID, ops.TILE_EPI_SWIGLU8
KINDS = {"qkv_rope_rs": ROPE, "o_down_resid": RESID, "gate_up_swiglu8_rs": SWIGLU8}


class _Form:
    """ops.TILE_PERSIST / TILE_PERSIST_CUS for the length of a with-block."""

    def __init__(self, persist, cus=0):
        self.new = (persist, cus)

    def __enter__(self):
        self.old = (ops.TILE_PERSIST, ops.TILE_PERSIST_CUS)
        ops.TILE_PERSIST, ops.TILE_PERSIST_CUS = self.new

    def __exit__(self, *exc):
        ops.TILE_PERSIST, ops.TILE_PERSIST_CUS = self.old


@pytest.fixture(scope="module")
def cos_sin():
    return ref.rope_cos_sin(4096, 128, 500000.0).to(DEV).float().contiguous()


def _guarded(rows, cols, dtype=torch.bfloat16):
    return torch.full((rows + 1, cols), NAN, device=DEV, dtype=dtype)


def _launch(epi, M, N, K, cs, seed):
    """A closure running the launch into fresh guarded buffers; returns the named outputs (with guard rows)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    if epi == RESID:
        wp = ops.pack_skinny(w)
        resid0 = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
        nw = (torch.rand(N, device=DEV, generator=g) + 0.5).to(torch.bfloat16)

        def run(packed):
            r, h, s = _guarded(M, N), _guarded(M, N), _guarded(M, N // 128, torch.float32)
            r[:M] = resid0
            ops.gemm_tile_resid(x, wp if packed else w, r[:M], nw, hw=h[:M], ss=s[:M])
            return {"resid": r, "hw": h, "ss_out": s}
        return run
    ss = (torch.rand(M, K // 128, device=DEV, generator=g) * 128 + 64).contiguous()
    if epi == ROPE:
        pos = ((torch.arange(M, device=DEV) * 37 + 11) % 4096).to(torch.int32)
        wp = ops.pack_skinny(w)

        def run(packed):
            y = _guarded(M, N)
            ops.gemm_tile(x, wp if packed else w, out=y[:M], algo=1, rope=(pos, cs, N // 128 - 1), rowscale=(ss, 1e-5))
            return {"y": y}
        return run
    w8 = ops.interleave_gate_up8(w).contiguous()
    wp = ops.pack_skinny(w8)

    def run(packed):
        y = _guarded(M, N // 2)
        ops.gemm_tile(x, wp if packed else w8, swiglu=8, out=y[:M], algo=1, rowscale=(ss, 1e-5))
        return {"y": y}
    return run


def _cases():
    out = []
    for name, epi in KINDS.items():
        ks = (192, 256, 4096) if epi == RESID else (512, 4096)
        for M in (512, 700):
            for N in (512, 768):
                for K in ks:
                    out.append(pytest.param(epi, M, N, K, id=f"{name}-M{M}-N{N}-K{K}"))
    out.append(pytest.param(RESID, 700, 768, 14336, id="o_down_resid-M700-N768-K14336"))
    return out


@pytest.mark.parametrize("epi,M,N,K", _cases())
def test_persistent_equals_one_tile_form_bitwise(epi, M, N, K, cos_sin):
    rs_np = 0 if epi == RESID else K // 128
    tiles = -(-M // 256) * (N // 256)
    plan = ops.native().gemm_tile_plan(0, M, N, K, epi, 1, 0, rs_np, persist=1, cus=3, ext=True)
    assert plan[0] == 0 and plan[6] >= 0 and (plan[5], plan[7]) == (tiles, 3), plan
    assert ops.native().gemm_tile_plan(0, M, N, K, epi, 1, 0, rs_np, persist=0, cus=3, ext=True)[6] == -1
    run = _launch(epi, M, N, K, cos_sin, seed=M + N + K)
    for packed in (False, True):  # row-major W and the fragment-packed layout
        with _Form(0):
            one = run(packed)
        with _Form(1, 3):
            per = run(packed)
        torch.cuda.synchronize()
        for name, a in one.items():
            b = per[name]
            what = f"{name} (packed={packed})"
            assert not torch.isnan(a[:M].float()).any(), f"one-tile form, {what}: a due store is missing"
            assert not torch.isnan(b[:M].float()).any(), f"persistent form, {what}: a due store is missing"
            assert torch.isnan(b[M].float()).all(), f"persistent form, {what}: the guard row was written"
            assert torch.equal(a[:M], b[:M]), f"{what}: {(a[:M] != b[:M]).sum().item()} elements differ"


def test_persistent_against_fp32_linear():
    """resid = 0 and norm_w = 1: resid and hw come out as bf16(x . w^T)."""
    M, N, K = 700, 768, 4096
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    resid = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    with _Form(1, 3):
        hw, ss = ops.gemm_tile_resid(x, w, resid, torch.ones(N, device=DEV, dtype=torch.bfloat16))
    r32 = torch.nn.functional.linear(x.cpu().float(), w.cpu().float())
    for name, t in (("resid", resid), ("hw", hw)):
        err = (t.cpu().float() - r32).abs()
        bad = (err > 3e-2 + 2e-2 * r32.abs()).sum().item()
        assert bad == 0, f"{name}: {bad} elements out of tolerance, max err {err.max().item():.4g}"
    ss32 = (resid.cpu().float() ** 2).view(M, N // 128, 128).sum(2)
    assert torch.allclose(ss.cpu(), ss32, rtol=1e-4, atol=1e-3)
