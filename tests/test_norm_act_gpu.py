"""The norm, activation and gather kernels of ops/csrc/norm_act.hip at every compiled form, loop
path and input edge, against the exact fp64 models and the one comparison rule of
tests/exact_small_ops.py (c = 8; tests/test_small_ops_models_cpu.py runs the same cases through
the CPU reference at c = 1)."""
import pytest
import torch

import exact_small_ops as X
from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = X.C_GPU


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()  # fail loudly when the extension is missing on a GPU box


# d -> NC of rmsnorm_kernel<NC, ADD>: 8..2048 -> 1, 2056 / 4096 -> 2 (2056: one vector in the second
# chunk), 5120 / 6144 / 8192 -> 4 (third chunk half full / fourth idle / all full), 8200 / 16384 -> 8
@pytest.mark.parametrize("d,family,fused", [(d, fam, fused) for fused in (False, True) for d in X.RMS_D
                                             for fam in (X.FUSED_FAMILIES if fused else X.NORM_FAMILIES)])
def test_rms_norm(d, family, fused):
    print(f"needs c={X.check_rms_norm(DEV, C, d, family, fused):.3g}")


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("d", [8, 2056, 8200])
def test_rms_norm_strided_rows(d, fused):
    print(f"needs c={X.check_rms_norm_strided(DEV, C, d, fused):.3g}")


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("d", [16392, 100])
def test_rms_norm_refuses(d, fused):
    """Wider than the NC = 8 form, or not a multiple of the 8-element vector: raises, writes nothing."""
    x = torch.ones(2, d, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(d, device=DEV, dtype=torch.bfloat16)
    res = torch.full((2, d), 3.0, device=DEV, dtype=torch.bfloat16)
    out = torch.full((2, d), 7.0, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        if fused:
            ops.fused_add_rms_norm(x, res, w, 1e-5, out=out)
        else:
            ops.rms_norm(x, w, 1e-5, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((res == 3.0).all())


@pytest.mark.parametrize("family", X.LN_FAMILIES)
@pytest.mark.parametrize("d", X.LN_D)
def test_layer_norm(d, family):
    print(f"needs c={X.check_layer_norm(DEV, C, d, family):.3g}")


def test_layer_norm_refuses():
    d = 8200
    x = torch.ones(2, d, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(d, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.layer_norm(x, w, w, 1e-5)


@pytest.mark.parametrize("F,interleaved", X.SILU_CASES)
def test_silu_mul(F, interleaved):
    print(f"needs c={X.check_silu_mul(DEV, C, F, interleaved):.3g}")


@pytest.mark.parametrize("rows,F,interleaved", X.SILU_LONG)
def test_silu_mul_row_loop(rows, F, interleaved):
    """More rows than grid.y holds (65535): the kernel's row loop runs a second pass."""
    print(f"needs c={X.check_silu_mul_long(DEV, C, rows, F, interleaved):.3g}")


@pytest.mark.parametrize("interleaved", [False, True])
def test_silu_mul_gate_sweep(interleaved):
    """Gates at both ends of exp's fp32 range against small, negative and large ups: no NaN, and
    every product within the rule (gate -100 x up 1e4 is a normal number, -3.7e-38)."""
    print(f"needs c={X.check_silu_mul_sweep(DEV, C, interleaved):.3g}")


@pytest.mark.parametrize("n", X.GELU_N)
def test_gelu(n):
    print(f"needs c={X.check_gelu(DEV, C, n):.3g}")


def test_gelu_sweep():
    print(f"needs c={X.check_gelu_sweep(DEV, C):.3g}")


@pytest.mark.parametrize("d", X.EMB_D)
def test_embedding(d):
    X.check_embedding(DEV, d)


@pytest.mark.parametrize("n", X.RESOLVE_N)
def test_resolve_ids(n):
    X.check_resolve_ids(DEV, n)
