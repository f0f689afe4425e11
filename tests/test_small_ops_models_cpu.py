"""The exact models of tests/exact_small_ops.py against ops.* on CPU tensors (= ops/reference.py),
over every case list the GPU tests run, under the same rule with c = 1 (the GPU tests allow c = 8).

This validates the models and the case generators without a GPU and pins the CPU execution path.
Each test prints the c the fp32 reference needed, so the margin of the GPU bound stays visible
(pytest -s).  The one place where the two may legitimately differ is the tie order of torch.topk in
ref.moe_route: rows whose fp32 softmax has equal values among its K + 1 largest are left out of the
id comparison on this side only (exact_small_ops.ref_tied_rows); the untied generator leaves out 0.
"""
import math

import pytest
import torch

import exact_small_ops as X
from k8s_llm_monitor_amd import ops

CPU = "cpu"
C = X.C_REF


def test_halfulp_bf16():
    r = torch.tensor([0.0, 1.0, 1.5, 1.9999, 2.0, -3.0, 0.75, 2.0 ** -126, 2.0 ** -130, 1e-41], dtype=torch.float64)
    want = [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -9, 2.0 ** -134, 2.0 ** -134, 2.0 ** -134]
    assert X.halfulp_bf16(r).tolist() == want
    # the nearest bf16 of any fp64 value is within the rule at c = 0, the next one over is not
    v = torch.randn(4096, dtype=torch.float64, generator=X.gen("halfulp")) * 37.0
    y = v.float().to(torch.bfloat16)
    assert X.fails_rule(y, v, v.abs(), 1.0) == 0  # fp64 -> fp32 -> bf16 double rounding: 2^-24 |v| at most
    up = torch.nextafter(y, torch.full_like(y, math.inf))
    dn = torch.nextafter(y, torch.full_like(y, -math.inf))
    far = torch.where((up.double() - v).abs() > (dn.double() - v).abs(), up, dn)
    assert X.fails_rule(far, v, v.abs(), 8.0) == 4096


def test_rule_rejects_nan_and_inf():
    r = torch.tensor([1.0, 2.0], dtype=torch.float64)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(AssertionError):
            X.assert_rule(torch.tensor([1.0, bad]).to(torch.bfloat16), r, r.abs(), 8.0, "x")


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("d", X.RMS_D)
def test_rms_norm_reference(d, fused):
    used = max(X.check_rms_norm(CPU, C, d, fam, fused) for fam in (X.FUSED_FAMILIES if fused else X.NORM_FAMILIES))
    print(f"rms_norm d={d} fused={fused}: reference needs c={used:.3g}")


@pytest.mark.parametrize("fused", [False, True])
def test_rms_norm_strided_reference(fused):
    for d in (8, 2056, 8200):
        X.check_rms_norm_strided(CPU, C, d, fused)


def test_fused_add_case_tells_rounded_from_unrounded_sum():
    """With residual ~ 256 randn and x ~ randn the bf16 rounding of the sum moves it by up to 1;
    a norm taken from the unrounded sum is then far outside the rule."""
    for d in (8, 2056):
        g = X.gen("discriminate", d)
        x = torch.randn(3, d, generator=g).to(torch.bfloat16)
        res = (256.0 * torch.randn(3, d, generator=g)).to(torch.bfloat16)
        w = torch.randn(d, generator=g).to(torch.bfloat16)
        good, _ = X.fused_add_rms_norm_model(x, res, w, 1e-5, rounded=True)
        wrong, _ = X.fused_add_rms_norm_model(x, res, w, 1e-5, rounded=False)
        y = ops.fused_add_rms_norm(x, res.clone(), w, 1e-5)
        assert X.fails_rule(y, good, good.abs(), X.C_GPU) == 0
        assert X.fails_rule(y, wrong, wrong.abs(), X.C_GPU) > 0.2 * y.numel()
        # and the other way round: the wrong computation, rounded once, fails the right model
        assert X.fails_rule(wrong.float().to(torch.bfloat16), good, good.abs(), X.C_GPU) > 0.2 * y.numel()


def test_eps_cases_tell_eps_values_apart():
    """Rows of scale 1e-3: a tenfold error in eps, or a dropped eps, moves most outputs out of the rule."""
    g = X.gen("eps")
    x, _ = X.norm_input("small_eps5", 3, 2056, g)
    w = torch.randn(2056, generator=g).to(torch.bfloat16)
    r = X.rms_norm_model(x, w, 1e-5)
    for wrong in (1e-6, 0.0):
        y = ops.rms_norm(x, w, wrong)
        assert X.fails_rule(y, r, r.abs(), X.C_GPU) > 0.5 * y.numel()


@pytest.mark.parametrize("d", X.LN_D)
def test_layer_norm_reference(d):
    used = max(X.check_layer_norm(CPU, C, d, fam) for fam in X.LN_FAMILIES)
    print(f"layer_norm d={d}: reference needs c={used:.3g}")


@pytest.mark.parametrize("F,interleaved", X.SILU_CASES)
def test_silu_mul_reference(F, interleaved):
    print(f"silu_mul F={F} il={interleaved}: reference needs c={X.check_silu_mul(CPU, C, F, interleaved):.3g}")


@pytest.mark.parametrize("rows,F,interleaved", X.SILU_LONG)
def test_silu_mul_long_reference(rows, F, interleaved):
    print(f"silu_mul rows={rows}: reference needs c={X.check_silu_mul_long(CPU, C, rows, F, interleaved):.3g}")


@pytest.mark.parametrize("interleaved", [False, True])
def test_silu_mul_gate_sweep_reference(interleaved):
    print(f"silu_mul sweep: reference needs c={X.check_silu_mul_sweep(CPU, C, interleaved):.3g}")


@pytest.mark.parametrize("n", X.GELU_N)
def test_gelu_reference(n):
    print(f"gelu n={n}: reference needs c={X.check_gelu(CPU, C, n):.3g}")


def test_gelu_sweep_reference():
    print(f"gelu sweep: reference needs c={X.check_gelu_sweep(CPU, C):.3g}")


@pytest.mark.parametrize("d", X.EMB_D)
def test_embedding_reference(d):
    X.check_embedding(CPU, d)


@pytest.mark.parametrize("n", X.RESOLVE_N)
def test_resolve_ids_reference(n):
    X.check_resolve_ids(CPU, n)


@pytest.mark.parametrize("family", X.ROUTE_FAMILIES)
@pytest.mark.parametrize("E,K", X.ROUTE_EK)
def test_moe_route_reference(E, K, family):
    left_out = X.check_moe_route(CPU, E, K, family)
    print(f"moe_route E={E} K={K} {family}: {left_out} tied rows left out of the id comparison")
    if family in X.ROUTE_UNTIED:
        assert left_out == 0


def test_moe_route_model_takes_lowest_index_among_equals():
    lg = torch.tensor([[1.0, 3.0, 3.0, 1.0, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0],
                       [-math.inf, 2.0, -math.inf, 2.0, -math.inf]])
    ids, w = X.moe_route_model(lg, 4, False)
    assert ids.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3], [1, 3, 0, 2]]
    assert w[2].tolist() == [0.5, 0.5, 0.0, 0.0]


@pytest.mark.parametrize("E", X.ROUTER_E)
@pytest.mark.parametrize("d", X.ROUTER_D)
def test_moe_router_reference(d, E):
    X.check_moe_router(CPU, d, E)


@pytest.mark.parametrize("E", X.ALIGN_E)
@pytest.mark.parametrize("n", X.ALIGN_N)
def test_moe_align_reference(n, E):
    X.check_moe_align(CPU, n, E)


@pytest.mark.parametrize("E", X.ALIGN_E)
def test_moe_align_one_pair_per_expert_reference(E):
    X.check_moe_align_one_each(CPU, E)


def test_align_invariants_reject_an_unstable_sort():
    ids = torch.tensor([1, 0, 1, 0], dtype=torch.int32)
    off, srt, inv = X.moe_align_model(ids, 2)
    assert (off.tolist(), srt.tolist(), inv.tolist()) == ([0, 2, 4], [1, 3, 0, 2], [2, 0, 3, 1])
    X.assert_align_invariants(ids, 2, off, srt, inv)
    bad = torch.tensor([3, 1, 0, 2], dtype=torch.int32)
    with pytest.raises(AssertionError):
        X.assert_align_invariants(ids, 2, off, bad, torch.tensor([2, 1, 3, 0], dtype=torch.int32))


@pytest.mark.parametrize("div", X.GATHER_DIV)
@pytest.mark.parametrize("d", X.GATHER_D)
def test_gather_rows_reference(d, div):
    X.check_gather_rows(CPU, d, div)


@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("K", X.COMBINE_K)
def test_moe_combine_reference(K, renorm):
    used = max(X.check_moe_combine(CPU, C, d, K, renorm) for d in X.GATHER_D)
    print(f"moe_combine K={K} renorm={renorm}: reference needs c={used:.3g}")


@pytest.mark.parametrize("T,K", [(2053, 1), (1027, 2)])
def test_moe_chain_reference(T, K):
    print(f"chain T={T} K={K}: reference needs c={X.check_moe_chain(CPU, C, T, K):.3g}")
