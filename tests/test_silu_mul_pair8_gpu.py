"""silu_mul over the [8 gate | 8 up] per-16 pairing (norm_act.hip silu_mul_kernel<8>,
ops.silu_mul(pairing=8)): the unfused activation behind a plain GEMM over a PACKED w13.

F in {8, 200, 1024} (one thread; no multiple of 64 or of a 256-thread block's 2048 features; a whole
block), rows in {1, 17}; gates include values below -87 (the split-exponent path) next to ordinary
ones.  Both kernels do the same arithmetic per element, so the result is bit-identical to
silu_mul(interleaved=False) over the de-interleaved input; guard rows around the output stay."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("rows", [1, 17])
@pytest.mark.parametrize("F", [8, 200, 1024])
def test_pair8_is_bit_identical_to_the_plain_pairing(F, rows):
    ops.native()
    g = torch.Generator(device=DEV).manual_seed(F * 31 + rows)
    gu = torch.randn(rows, 2 * F, device=DEV, generator=g) * 3.0  # [F gate | F up]
    gu[:, 0:F:5] = -88.0 - 8.0 * torch.rand(rows, len(range(0, F, 5)), device=DEV, generator=g)  # gates below -87
    gu[:, F:2 * F:5] = 2.0e4  # large ups beside them: silu(-96) * 2e4 = -3.9e-36 is a normal number
    gu = gu.to(torch.bfloat16)
    assert bool((gu[:, :F] < -87).any()) and bool((gu[:, :F] > -87).any())
    x8 = ops.interleave_gate_up8(gu.t().contiguous()).t().contiguous()
    # the pairing as the issue states it: feature c's gate at column 2 (c - c % 8) + c % 8, its up 8 further
    c = torch.arange(F, device=DEV)
    assert torch.equal(x8[:, 2 * (c - c % 8) + c % 8], gu[:, :F]) and torch.equal(x8[:, 2 * (c - c % 8) + c % 8 + 8], gu[:, F:])
    want = ops.silu_mul(gu, interleaved=False)
    buf = torch.full((rows + 2, F), 7.5, device=DEV, dtype=torch.bfloat16)
    out = ops.silu_mul(x8, out=buf[1:rows + 1], pairing=8)
    assert out.data_ptr() == buf[1:].data_ptr()
    assert bool((buf[0] == 7.5).all()) and bool((buf[rows + 1] == 7.5).all()), "guard rows changed"
    assert torch.equal(buf[1:rows + 1], want)
    assert torch.equal(ops.silu_mul(x8, pairing=8), want)
    # the CPU reference of the new pairing is the plain one's over the de-interleaved input too
    assert torch.equal(ref.silu_mul(x8.cpu(), pairing=8), ref.silu_mul(gu.cpu()))
    low = (gu[:, :F] < -87).cpu()
    assert bool((want.cpu()[low] != 0).any()), "the gates below -87 must not all flush to zero"


def test_native_forms_stay():
    ops.native()
    x = (torch.randn(3, 256, device=DEV) * 2).to(torch.bfloat16)
    a, b = torch.empty(3, 128, device=DEV, dtype=torch.bfloat16), torch.empty(3, 128, device=DEV, dtype=torch.bfloat16)
    ops.native().silu_mul(a, x, False)
    ops.native().silu_mul_pairing(b, x, 0)
    assert torch.equal(a, b)
    ops.native().silu_mul(a, x, True)
    ops.native().silu_mul_pairing(b, x, 1)
    assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="pairing"):
        ops.native().silu_mul_pairing(b, x, 4)
    with pytest.raises(ValueError, match="pairing"):
        ops.silu_mul(x, pairing=16)
