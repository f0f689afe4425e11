"""The plan is what the launch does: native().gemm_dec (the one binding of the shared-A decode GEMM)
against native().gemm_dec_plan and against the public wrappers, for bf16 / fp8 / mxfp4 weights, dense
and grouped (E = 2) launches.

Per case the first row of ops.DEC_FORMS whose plan accepts the launch, at N = 16 ntw waves (for the
SwiGLU epilogue times 4 where that is no multiple of 64: its packed output holds whole 32-feature
k-steps), K = 512 in 1 or 2 slices (256 per slice; only slabs split); 1, 17 and 64 rows, dense also
65 and 128.  Weight row r is multiplied by 2^(r % 5 - 2) before encoding and the routing weights
have zeros, so a scale, an expert or a row order read wrong cannot pass.  Asserted per launch:
  1. the returned slab count is the plan's, and the plan's grid is (column groups, splits, experts);
  2. bit equality (torch.equal) with the public wrapper's launch of the same ``cfg``, and for fp8 and
     mxfp4 also with the bf16 wrapper's launch over the dequantised weights (the codes convert
     exactly and the power-of-two scales commute with every rounding); for bf16 the project's bound
     against the fp32 product, 2.5e-2 * scale + 1e-3, so the comparison is not only with itself;
  3. every element of the output written, and the NaN-poisoned, over-allocated workspace / output
     untouched just past it."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 512
PAD = 256  # poisoned elements past every output
WF = {None: 0, "fp8": 1, "mxfp4": 2}


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    _weights.cache_clear()


@functools.lru_cache(maxsize=None)
def _weights(N, enc, il, E):
    """Per expert (dense: one): (values [N, K] bf16 in canonical row order - the dequantised ones for
    a quantised ``enc`` -, packed bf16 weight, packed codes, packed scales); ``il``: [gate; up] rows,
    packed in the [8 gate | 8 up] order."""
    out = []
    for e in range(max(E, 1)):
        g = torch.Generator(device=DEV).manual_seed(9000 + 31 * e + N)
        w = torch.randn(N, K, device=DEV, generator=g) * 0.02
        w = (w * torch.exp2(((torch.arange(N, device=DEV) + e) % 5 - 2).float())[:, None]).to(torch.bfloat16)
        qp = sp = None
        if enc:
            w, qp, sp = ops.encode_weight(w, enc, gate_up8=il)
        out.append((w, ops.pack_skinny(ops.interleave_gate_up8(w) if il else w), qp, sp))
    if not E:
        return out[0]
    return tuple(None if t[0] is None else torch.stack(t).contiguous() for t in zip(*out))


def _x(M, e=0):
    g = torch.Generator(device=DEV).manual_seed(M * 7919 + 131 * e)
    return torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)


def _first_form(enc, E, epi, M, S, rw):
    for f in ops.DEC_FORMS:
        if f[0] != epi:
            continue
        N = 16 * f[1] * f[2]
        N *= 4 if epi == ops.DEC_SWIGLU8 and N % 64 else 1
        plan = ops.native().gemm_dec_plan(WF[enc], M, N, K, S, epi, *f[1:4], 0, E, rw, 0)
        if plan[0] == 0:
            return f, N, plan
    return None, 0, None


def _outputs(epi, E, S, M, N):
    """NaN-poisoned (workspace, out, the written part as a view, the part past it)."""
    g = (E,) if E else ()
    if epi == ops.DEC_SLAB:
        n = max(E, 1) * S * M * N
        ws = torch.full((n + PAD,), float("nan"), device=DEV, dtype=torch.float32)
        return ws, None, ws[:n], ws[n:]
    if epi == ops.DEC_BF16:
        y = torch.full((M + 2, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        return None, y, y[:M], y[M:]
    shape = g + (-(-M // 16), N // 64, 64, 8)
    n = torch.Size(shape).numel()
    buf = torch.full((n + PAD,), float("nan"), device=DEV, dtype=torch.bfloat16)
    return None, buf[:n].view(shape), buf[:n].view(shape), buf[n:]


def _rows_of(epi, E, M, written):
    """The written part as comparable rows: SwiGLU outputs unpacked to their M valid rows."""
    if epi != ops.DEC_SWIGLU8:
        return written
    return torch.stack([ops.unpack_skinny(t)[:M] for t in (written if E else written[None])])


def _case(enc, E, epi, M, S):
    nat = ops.native()
    rw_on = bool(E) and epi == ops.DEC_SLAB
    form, N, plan = _first_form(enc, E, epi, M, S, rw_on)
    if form is None:
        return False
    cfg = (S,) + form[1:4]
    il = epi == ops.DEC_SWIGLU8
    vals, wp, qp, sp = _weights(N, enc, il, E)
    w, wscale = (qp, sp) if enc else (wp, None)
    per_e = bool(E) and epi == ops.DEC_SLAB  # down: A per expert; gate_up: A shared
    xs = [_x(M, e) for e in range(E)] if per_e else [_x(M)]
    a = torch.stack([ops.pack_activation(x) for x in xs]) if per_e else ops.pack_activation(xs[0])
    row_w = None
    if rw_on:  # routing weights with zeros: row m skips expert m % E
        row_w = torch.rand(M, E, device=DEV, generator=torch.Generator(device=DEV).manual_seed(77 + M)) + 0.25
        row_w[torch.arange(M, device=DEV), torch.arange(M, device=DEV) % E] = 0.0
    what = f"{enc or 'bf16'} E={E} form={form} rows={M} S={S}"

    def launch(fn):
        ws, out, written, tail = _outputs(epi, E, S, M, N)
        r = fn(ws, out)
        got = _rows_of(epi, E, M, written)
        assert not torch.isnan(got).any(), f"{what}: every element written"
        assert torch.isnan(tail).all(), f"{what}: nothing written past the output"
        return r, got.clone()

    r, got = launch(lambda ws, out: nat.gemm_dec(a, w, wscale, ws, out, S, epi, *form[1:4], M, None, 0.0, row_w, 0))
    assert r == plan[8] == (max(E, 1) * S if epi == ops.DEC_SLAB else 1), what
    assert tuple(plan[5:8]) == (-(-N // (16 * form[1] * form[2])), S, max(E, 1)) and plan[1] == -(-M // 16), what

    def wrapper(quant):
        def fn(ws, out):
            if not E:
                return ops.dec_gemm(a, w if quant else wp, epi, M, workspace=ws, out=out, cfg=cfg,
                                    wscale=wscale if quant else None)
            if quant:
                return ops.dec_gemm_grouped_q(a, qp, sp, epi, M, workspace=ws, out=out, row_w=row_w, cfg=cfg)
            return ops.dec_gemm_grouped(a, wp, epi, M, workspace=ws, out=out, row_w=row_w, cfg=cfg)
        return fn

    for quant in ((True, False) if enc else (False,)):
        r2, ref = launch(wrapper(quant))
        assert r2 == r and torch.equal(got, ref), f"{what}: differs from the {'same' if quant or not enc else 'bf16'} wrapper launch"
    if enc is None:  # against the fp32 product
        for e in range(max(E, 1)):
            y = (xs[e if per_e else 0].float() @ (vals[e] if E else vals).float().t())
            if epi == ops.DEC_SLAB:
                have = got.view(max(E, 1), S, M, N)[e].sum(0)
                y = y * row_w[:, e:e + 1] if row_w is not None else y
            elif epi == ops.DEC_BF16:
                have = got.float()
            else:
                y = torch.nn.functional.silu(y[:, : N // 2].to(torch.bfloat16).float()) * y[:, N // 2:].to(torch.bfloat16).float()
                have = got[e].float()
            assert (have - y).abs().max() <= 2.5e-2 * y.abs().max() + 1e-3, what
    return True


@pytest.mark.parametrize("E", [0, 2], ids=["dense", "grouped"])
@pytest.mark.parametrize("enc", [None, "fp8", "mxfp4"], ids=["bf16", "fp8", "mxfp4"])
def test_the_plan_is_what_the_launch_does(enc, E):
    ran = {}
    for M in (1, 17, 64) + (() if E else (65, 128)):
        for epi, splits in ((ops.DEC_SLAB, (1, 2)), (ops.DEC_SWIGLU8, (1,))) + (() if E else ((ops.DEC_BF16, (1,)),)):
            for S in splits:
                ran[(epi, M, S)] = _case(enc, E, epi, M, S)
    torch.cuda.synchronize()
    # every format has a slab and a SwiGLU row for every one of these row counts, and a bf16-output row
    assert all(ok for (epi, _, _), ok in ran.items()), [k for k, ok in ran.items() if not ok]
