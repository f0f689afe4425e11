"""The MoE dispatch kernels of ops/csrc/moe.hip (route, router, align, gather_rows, combine) at every
compiled form, loop path and input edge, against the exact models of tests/exact_small_ops.py:
expert ids, moe_align's outputs and gathered rows bit for bit, routing weights at the project's
fp32 tolerance, combined rows under the comparison rule (c = 8).  No test hands an id outside
[0, E) to a kernel."""
import pytest
import torch

import exact_small_ops as X
from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = X.C_GPU


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()


@pytest.mark.parametrize("family", X.ROUTE_FAMILIES)
@pytest.mark.parametrize("E,K", X.ROUTE_EK)
def test_moe_route(E, K, family):
    """T on both sides of the 256-thread block edge, renorm on and off; ties go to the lowest index."""
    assert X.check_moe_route(DEV, E, K, family) == 0  # every row's ids are compared


@pytest.mark.parametrize("E,K", [(65, 2), (8, 9)])
def test_moe_route_refuses(E, K):
    with pytest.raises(RuntimeError):
        ops.moe_route(torch.zeros(4, E, device=DEV), K, True)


@pytest.mark.parametrize("E,K", [(8, 2), (64, 8), (5, 5)])
def test_moe_route_nan_row_picks_valid_experts(E, K):
    """A row of NaN logits (no comparison holds) still gets K distinct experts of [0, E), and the
    healthy rows are what they are when routed alone.  The ids go nowhere else."""
    T = 6
    lg = 2.0 * torch.randn(T, E, generator=X.gen("nan", E, K))
    lg[2] = float("nan")
    ids, w = ops.moe_route(lg.to(DEV), K, True)
    ids, w = ids.cpu(), w.cpu()
    assert bool(((ids >= 0) & (ids < E)).all())
    assert all(len(set(r)) == K for r in ids.tolist())
    keep = torch.tensor([0, 1, 3, 4, 5])
    ids2, w2 = ops.moe_route(lg[keep].to(DEV), K, True)
    assert torch.equal(ids[keep], ids2.cpu()) and torch.equal(w[keep], w2.cpu())
    mids, mw = X.moe_route_model(lg[keep], K, True)
    assert torch.equal(ids[keep], mids)


@pytest.mark.parametrize("E", X.ROUTER_E)
@pytest.mark.parametrize("d", X.ROUTER_D)
def test_moe_router(d, E):
    """Both EMAX forms and their boundary (E = 8 | 9), d below, at and between whole passes of the
    256 x 8 column loop, K in {1, 2, E}, renorm on and off: ids, w and the dense wd (zeros included)
    against the exact model - not against ops.moe_route."""
    assert X.check_moe_router(DEV, d, E) == 0


@pytest.mark.parametrize("E", X.ALIGN_E)
@pytest.mark.parametrize("n", X.ALIGN_N)
def test_moe_align(n, E):
    """C = ceil(n / 1024) items per thread from 1 to 128; uniform ids, all pairs to the first / the
    last expert, the first and the last expert empty."""
    X.check_moe_align(DEV, n, E)


@pytest.mark.parametrize("E", X.ALIGN_E)
def test_moe_align_one_pair_per_expert(E):
    X.check_moe_align_one_each(DEV, E)


@pytest.mark.parametrize("div", X.GATHER_DIV)
@pytest.mark.parametrize("d", X.GATHER_D)
def test_gather_rows(d, div):
    X.check_gather_rows(DEV, d, div)


@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("K", X.COMBINE_K)
@pytest.mark.parametrize("d", X.GATHER_D)
def test_moe_combine(d, K, renorm):
    print(f"needs c={X.check_moe_combine(DEV, C, d, K, renorm):.3g}")


@pytest.mark.parametrize("T,K", [(2053, 1), (1027, 2)])
def test_route_align_gather_combine_returns_the_rows(T, K):
    """T * K = 2053 (and 2054): moe_align's per-thread count C > 1 flows through the whole chain."""
    print(f"needs c={X.check_moe_chain(DEV, C, T, K):.3g}")
