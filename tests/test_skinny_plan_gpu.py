"""The launch plan of the skinny decode GEMM (csrc/gemm_skinny_plan.h) on the GPU: the slab count
the bindings report is the count the kernel writes, and every row of kSkinnyForms
(native().gemm_skinny_forms()) launched at its smallest and largest m-tile count (rows = 16 mt - 3)
on the smallest shape that makes skinny_plan pick it, against the fp32 product at the tolerances of
tests/test_skinny_rm_gpu.py.  Driven by the table: a form added to it is covered without an edit
here.  (The 2-versus-4-wave rule of the row-major kernel flips above 256 workgroups: covered by
comparing plans on the CPU, not by a big launch; its forms are reached with SKINNY_WAVES_FORCE.)"""
import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F_ = torch.nn.functional
SLAB, BF16, SWIGLU, SWIGLU_PACKED = 0, 1, 2, 3
PACKED, RM = 0, 1
FORMS = [tuple(f) for f in ops.native().gemm_skinny_forms()] if ops.native_available() else []


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()


def _close(a, b, what, atol=3e-2, rtol=2e-2):
    err = (a.float() - b.float()).abs()
    bad = (err > atol + rtol * b.float().abs()).sum().item()
    print(f"{what}: max err {err.max().item():.4g}")
    assert bad == 0, f"{what}: {bad} elements out of tolerance, max err {err.max().item():.4g}"


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(torch.bfloat16)


def _swiglu_ref(x, w13):
    """silu(gate) * up with gate and up rounded to bf16 first, as the kernels do; w13 = [gate; up]."""
    g, u = F_.linear(x.float(), w13.float()).to(torch.bfloat16).float().chunk(2, dim=1)
    return F_.silu(g) * u


def _plan(M, N, K, S, epi, nt, a_packed, waves, experts, w_rm):
    return tuple(ops.native().gemm_skinny_plan(M, N, K, S, epi, nt, a_packed, waves, experts, w_rm))


def _written(ws, ns, M, N, what):
    """Slabs [0, ns) of a workspace pre-filled with 7.0 summed; nothing of the fill left in them,
    nothing but the fill behind them."""
    head, tail = ws[: ns * M * N], ws[ns * M * N:]
    assert not (head == 7.0).any(), f"{what}: {ns} slabs reported, not all of them written"
    assert (tail == 7.0).all(), f"{what}: written past the {ns} slabs reported"
    return head.view(ns, M, N).sum(0)


@pytest.mark.parametrize("M,N,K,S", [(5, 128, 256, 3), (20, 64, 1024, 5)])
def test_slab_count_is_what_the_kernel_writes(M, N, K, S):
    """Row-major weights slice K by 64-deep stages: 3 splits of K = 256 are two slices, 5 of 1024
    four.  The call reports the slabs the kernel wrote."""
    a, w = _randn(M, K, seed=M), _randn(N, K, seed=N, scale=0.05)
    ws = torch.full((S * M * N,), 7.0, device=DEV)
    ns = ops.skinny_slabs(ops.pack_activation(a), w, ws, S, rows=M)
    y = _written(ws, ns, M, N, f"M{M} N{N} K{K} S{S}")
    _close(y.cpu(), F_.linear(a.cpu().float(), w.cpu().float()), f"rm slabs M{M} N{N} K{K} S{S}")
    assert ns == _plan(M, N, K, S, SLAB, 4, 1, 0, 1, 1)[6] == ops.skinny_nslabs(K, S, rm=True) < S


def test_grouped_slab_count_is_what_the_kernel_writes():
    E, M, N, K, S = 2, 5, 64, 256, 3
    x, w = _randn(E, M, K, seed=1), _randn(E, N, K, seed=2, scale=0.05)
    wd = torch.rand(M, E, device=DEV)
    act = torch.stack([ops.pack_activation(x[e]) for e in range(E)])
    ws = torch.full((E * S * M * N,), 7.0, device=DEV)
    ns = ops.skinny_grouped_slabs(act, w, ws, M, wd, splits=S)
    y = _written(ws, ns, M, N, "grouped")
    ref = sum(F_.linear(x[e].cpu().float(), w[e].cpu().float()) * wd[:, e:e + 1].cpu() for e in range(E))
    _close(y.cpu(), ref, "rm grouped slabs")
    assert ns == E * _plan(M, N, K, S, SLAB, 4, 1, 0, E, 1)[6] == E * 2


def _run_form(form, mt):
    """One launch of `form` at mt m-tiles through the public ops; returns (result, fp32 reference)."""
    fam, epi, nt, waves, a_packed, min_mt, max_mt = form
    M, K = 16 * mt - 3, 256
    E = 2 if mt > 4 else 1  # above 64 rows: grouped launches only
    N = 192 if nt == 3 else 128  # 48-column tiles need 48 | N, and must not fire at nt 4
    S = 2 if epi == SLAB else 1
    plan = _plan(M, N, K, S, epi, 4 if nt == 3 else nt, a_packed, waves, E, fam)
    assert plan[:5] == (0, fam, mt, nt, waves) and plan[6] == S, f"{form} at {mt} m-tiles: plan {plan}"
    x = _randn(E, M, K, seed=mt)
    w = _randn(E, N, K, seed=100 + epi, scale=0.05)
    swiglu = epi in (SWIGLU, SWIGLU_PACKED)
    wk = torch.stack([ops.interleave_gate_up(we) for we in w]) if swiglu else w
    if fam == PACKED:
        wk = torch.stack([ops.pack_skinny(we) for we in wk])
    ref = [_swiglu_ref(x[e], w[e]) if swiglu else F_.linear(x[e].float(), w[e].float()) for e in range(E)]
    if E > 1:  # the grouped ops: SWIGLU_PACKED over a shared A, SLAB over per-expert A and routing weights
        if epi == SWIGLU_PACKED:
            act = ops.skinny_grouped_swiglu(ops.pack_activation(x[0]), wk.contiguous(), rows=M)
            return (torch.stack([ops.unpack_skinny(act[e])[:M] for e in range(E)]),
                    torch.stack([_swiglu_ref(x[0], w[e]) for e in range(E)]))
        wd = torch.rand(M, E, device=DEV)
        ws = torch.full((E * S * M * N,), 7.0, device=DEV)
        act = torch.stack([ops.pack_activation(x[e]) for e in range(E)])
        assert ops.skinny_grouped_slabs(act, wk.contiguous(), ws, M, wd, splits=S) == E * S
        return _written(ws, E * S, M, N, str(form)), sum(ref[e] * wd[:, e:e + 1] for e in range(E))
    a, wk = (ops.pack_activation(x[0]) if a_packed else x[0]), wk[0].contiguous()
    if epi == SLAB:
        ws = torch.full((S * M * N,), 7.0, device=DEV)
        assert ops.skinny_slabs(a, wk, ws, S, nt_tiles=4 if nt == 3 else nt, rows=M) == S
        return _written(ws, S, M, N, str(form)), ref[0]
    if epi == BF16:
        return ops.skinny_linear(a, wk, nt_tiles=nt, rows=M), ref[0]
    y = ops.skinny_swiglu(a, wk, rows=M, packed_out=epi == SWIGLU_PACKED)
    return (ops.unpack_skinny(y)[:M] if epi == SWIGLU_PACKED else y), ref[0]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "fam{}-epi{}-nt{}-w{}-ap{}-mt{}to{}".format(*f))
def test_skinny_form_matches_fp32(form, monkeypatch):
    monkeypatch.setattr(ops, "SKINNY_WAVES_FORCE", form[3])
    for mt in sorted({form[5], form[6]}):
        y, ref = _run_form(form, mt)
        _close(y.cpu(), ref.cpu(), f"{form} at {mt} m-tiles")
    torch.cuda.synchronize()
