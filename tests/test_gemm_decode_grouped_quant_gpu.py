"""Grouped (grid.z = expert) launches of the shared-A decode GEMM over fp8 and mxfp4 expert stacks
(ops.dec_gemm_grouped_q), for every SLAB and SWIGLU8 form of ops.DEC_F8_FORMS / ops.DEC_F4_FORMS with
``cfg`` passed explicitly.  E = 3 experts; K = 512 for gate_up (SWIGLU8, A shared by the experts) and
1024 for down (SLAB, A per expert; splits 1 and 2 - mxfp4 needs whole 256-deep slices); N =
64 (waves + 1) for SWIGLU8 (ragged last workgroup) and 16 waves 2 for SLAB; rows 1, 23 and 64.

Weight row r of expert e is multiplied by 2^((r + 3e) % 7 - 3) before quantising, so a scale or a
code read at the wrong expert or in the wrong row order cannot pass; ``row_w`` has zeros; outputs
and the workspace tail are NaN-filled.  Per launch:
  1. bit equality (torch.equal) with dec_gemm_grouped of the same ``cfg`` over the dequantised bf16
     stacks, slab by slab and expert by expert: the codes convert to bf16 exactly, the MFMA sequence
     is the same, and the power-of-two scales (on the fp32 accumulator for fp8, on the operand for
     mxfp4) commute with every rounding, the routing weight coming last in both;
  2. the project's bound against the fp32 product over the dequantised weights
     (2.5e-2 * scale + 1e-3);
  3. every slab element written, nothing past E * S * M * N touched;
  4. 65 rows refused before any launch;
  5. mxfp4 at <= 16 rows also with the ring depth forced to 8 and to 16."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F_ = torch.nn.functional
E = 3
K_UP, K_DOWN = 512, 1024
ROWS = (1, 23, 64)
_ID = "epi{}-ntw{}-w{}-d{}-mt{}-wide{}"
_GROUPED = (ops.DEC_SLAB, ops.DEC_SWIGLU8)
F8_FORMS = [ops.DEC_FORMS[i] for i in ops.DEC_F8_FORMS if ops.DEC_FORMS[i][0] in _GROUPED]
F4_FORMS = [ops.DEC_FORMS[i] for i, _ in ops.DEC_F4_FORMS if ops.DEC_FORMS[i][0] in _GROUPED]


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    _stack.cache_clear()


def _shape(epi, waves):
    return (64 * (waves + 1), K_UP) if epi == ops.DEC_SWIGLU8 else (16 * waves * 2, K_DOWN)


@functools.lru_cache(maxsize=None)
def _stack(N, K, enc, il):
    """E weights [N, K] (``il``: [gate; up] rows, encoded in interleave_gate_up8 order): (dequantised
    row-major [E, N, K] bf16 in the canonical row order, packed bf16 stack, code stack, scale stack)."""
    dqs, wps, qps, sps = [], [], [], []
    for e in range(E):
        g = torch.Generator(device=DEV).manual_seed(4000 + 17 * e + N + K)
        w = torch.randn(N, K, device=DEV, generator=g) * 0.02
        w = (w * torch.exp2(((torch.arange(N, device=DEV) + 3 * e) % 7 - 3).float())[:, None]).to(torch.bfloat16)
        w = ops.interleave_gate_up8(w) if il else w
        if enc == "fp8":
            q, s = ops.quantize_rows_fp8(w)
            dq = ops.dequantize_rows_fp8(q, s)
            qp, sp = ops.pack_skinny_f8(q), s.contiguous()
        else:
            q, s = ops.quantize_mxfp4(w)
            dq = ops.dequantize_mxfp4(q, s)
            qp, sp = ops.pack_skinny_f4(q, s)
        dqs.append(ops.deinterleave_gate_up8(dq) if il else dq)
        wps.append(ops.pack_skinny(dq))
        qps.append(qp)
        sps.append(sp)
    return tuple(torch.stack(t).contiguous() for t in (dqs, wps, qps, sps))


def _x(M, K, e=0):
    g = torch.Generator(device=DEV).manual_seed(M * 7919 + K + 131 * e)
    return torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)


def _row_w(M):
    """Routing weights [M, E] with zeros: row m skips expert m % E."""
    g = torch.Generator(device=DEV).manual_seed(77 + M)
    w = torch.rand(M, E, device=DEV, generator=g) + 0.25
    w[torch.arange(M, device=DEV), torch.arange(M, device=DEV) % E] = 0.0
    return w.contiguous()


def _launch(epi, cfg, N, K, M, a, enc, quant, row_w=None):
    """One grouped launch over NaN-filled outputs, over the codes (``quant``) or the bf16 stack of the
    same weights: SLAB -> [E, S, M, N] fp32, SWIGLU8 -> [E, M, N / 2] bf16."""
    S = cfg[0]
    _, wp, qp, sp = _stack(N, K, enc, epi == ops.DEC_SWIGLU8)

    def run(**kw):
        if quant:
            return ops.dec_gemm_grouped_q(a, qp, sp, epi, M, cfg=cfg, **kw)
        return ops.dec_gemm_grouped(a, wp, epi, M, cfg=cfg, **kw)

    if epi == ops.DEC_SLAB:
        n = E * S * M * N
        ws = torch.full((n + 64,), float("nan"), device=DEV, dtype=torch.float32)
        assert run(workspace=ws, row_w=row_w) == E * S
        assert not torch.isnan(ws[:n]).any(), "every slab element written"
        assert torch.isnan(ws[n:]).all(), "nothing written past the E * S * M * N slabs"
        return ws[:n].view(E, S, M, N)
    act = torch.full((E, -(-M // 16), N // 64, 64, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
    run(out=act)
    y = torch.stack([ops.unpack_skinny(act[e])[:M] for e in range(E)])
    assert not torch.isnan(y).any(), "every feature of every row of every expert written"
    return y


def _check_form(form, enc, rows=ROWS, what=""):
    epi, ntw, waves, depth, _, _ = form
    N, K = _shape(epi, waves)
    dq = _stack(N, K, enc, epi == ops.DEC_SWIGLU8)[0].float()
    for M in rows:
        if epi == ops.DEC_SWIGLU8:
            x = _x(M, K)
            a, rw = ops.pack_activation(x), None
            xs = [x.float()] * E
        else:
            xe = [_x(M, K, e) for e in range(E)]
            a, rw = torch.stack([ops.pack_activation(x) for x in xe]).contiguous(), _row_w(M)
            xs = [x.float() for x in xe]
        for S in ((1, 2) if epi == ops.DEC_SLAB else (1,)):
            cfg = (S, ntw, waves, depth)
            tag = f"{enc} {form} M{M} S{S}{what}"
            yq = _launch(epi, cfg, N, K, M, a, enc, True, rw)
            yb = _launch(epi, cfg, N, K, M, a, enc, False, rw)
            for e in range(E):
                for s in range(S if epi == ops.DEC_SLAB else 1):
                    q, b = (yq[e, s], yb[e, s]) if epi == ops.DEC_SLAB else (yq[e], yb[e])
                    diff = (q.float() - b.float()).abs().max().item()
                    print(f"{tag} expert {e} slab {s}: max diff to the bf16 launch {diff:.4g}")
                    assert torch.equal(q, b), f"{tag}: expert {e} slab {s} differs from the bf16 grouped launch ({diff:.4g})"
                if epi == ops.DEC_SLAB:
                    ref = (xs[e] @ dq[e].t()) * rw[:, e:e + 1]
                    y = yq[e].sum(0)
                    skipped = rw[:, e] == 0
                    assert torch.equal(y[skipped], torch.zeros_like(y[skipped])), f"{tag}: rows that skip expert {e} are 0"
                else:
                    g = (xs[e] @ dq[e, : N // 2].t()).to(torch.bfloat16).float()
                    u = (xs[e] @ dq[e, N // 2:].t()).to(torch.bfloat16).float()
                    ref = F_.silu(g) * u
                    y = yq[e].float()
                scale = ref.abs().max().item()
                err = (y - ref).abs().max().item()
                print(f"{tag} expert {e}: max err {err:.4g} scale {scale:.4g}")
                assert err <= 2.5e-2 * scale + 1e-3, f"{tag} expert {e}: max err {err:.4g} vs scale {scale:.4g}"
    torch.cuda.synchronize()


def _refused_at_65(form, enc):
    epi, ntw, waves, depth, _, _ = form
    N, K = _shape(epi, waves)
    x = ops.pack_activation(_x(65, K))
    a = x if epi == ops.DEC_SWIGLU8 else torch.stack([x] * E).contiguous()
    with pytest.raises((ValueError, RuntimeError), match="at most 64 rows"):
        _launch(epi, (1, ntw, waves, depth), N, K, 65, a, enc, True, None if epi == ops.DEC_SWIGLU8 else _row_w(65))
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", F8_FORMS, ids=lambda f: _ID.format(*f))
def test_grouped_fp8_bit_equal_to_bf16_and_within_bound(form):
    _check_form(form, "fp8")
    _refused_at_65(form, "fp8")


@pytest.mark.parametrize("form", F4_FORMS, ids=lambda f: _ID.format(*f))
def test_grouped_mxfp4_bit_equal_to_bf16_and_within_bound(form):
    _check_form(form, "mxfp4")
    _refused_at_65(form, "mxfp4")


@pytest.mark.parametrize("d4", (8, 16))
@pytest.mark.parametrize("form", F4_FORMS, ids=lambda f: _ID.format(*f))
def test_grouped_mxfp4_forced_ring_depth(form, d4, monkeypatch):
    """<= 16 rows: the ring depth the launcher would choose and the other one give the same bits."""
    assert ops.dec_f4_depth(form[0], (1,) + tuple(form[1:4])) >= d4
    monkeypatch.setattr(ops, "DEC_F4_DEPTH_FORCE", d4)
    _check_form(form, "mxfp4", rows=(1, 16), what=f" ring depth {d4}")


def test_forms_cover_both_epilogues():
    for forms in (F8_FORMS, F4_FORMS):
        assert {f[0] for f in forms} == set(_GROUPED)


def test_grouped_form_without_quantised_instantiation_raises_before_launch():
    for enc, have in (("fp8", F8_FORMS), ("mxfp4", F4_FORMS)):
        out = [f for f in ops.DEC_FORMS if f[0] in _GROUPED and f not in have]
        assert out, "some grouped form stays bf16-only"
        for epi, ntw, waves, depth, _, _ in out:
            N, K = _shape(epi, waves)
            x = ops.pack_activation(_x(1, K))
            a = x if epi == ops.DEC_SWIGLU8 else torch.stack([x] * E).contiguous()
            with pytest.raises(RuntimeError, match=f"over {enc} weights"):
                _launch(epi, (1, ntw, waves, depth), N, K, 1, a, enc, True)
    torch.cuda.synchronize()


def test_scale_stack_of_the_wrong_shape_is_refused():
    N, K = _shape(ops.DEC_SLAB, 8)
    for enc in ("fp8", "mxfp4"):
        _, _, qp, sp = _stack(N, K, enc, False)
        a = torch.stack([ops.pack_activation(_x(1, K))] * E).contiguous()
        ws = torch.empty(E * N, device=DEV, dtype=torch.float32)
        with pytest.raises(ValueError, match="needs its scales"):
            ops.dec_gemm_grouped_q(a, qp, sp[:2], 0, 1, workspace=ws, cfg=(1, 1, 8, 8))
