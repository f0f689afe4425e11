"""Every compiled form of the prefill tile GEMM, launched once per schedule through the public
wrappers (ops.gemm_tile / gemm_tile_resid): the walk is over ops.TILE_FORMS, so a new row is
covered without an edit here.

Shapes: M = 300 (two m-tiles, the second ragged); N = 512 for the SwiGLU forms, else 384 (a last
n-tile of 128 columns, one wave's quarter wholly past N - the case the RESID and ROPE epilogues
handle specially); K = 256, the least depth all three formats take (four k-tiles: every peeled tail
phase of schedule 1 and one steady iteration).  The row-scaled forms run at K = 512 instead: the
scale is read four K / 128 partial sums at a time, so 512 is the least K they take.  The rows that
have a schedule-0 twin run it at K = 256 (algo=0) and at K = 128 through algo=1, the fallback.
Grouped rows: E = 3 with 0, 300 and 45 rows (an empty expert and a ragged one) between rows that
belong to no expert.  Weights are those of tests/test_gemm_tile_f8_gpu.py / test_gemm_tile_f4_gpu.py;
the bf16 rows read the fp8 file's dequantised weight, row-major and fragment-packed.

Per launch, over NaN-filled outputs with one guard row: no NaN where a store is due; the guard row
and the rows outside the offsets untouched; the bound of tests/test_gemm_tile_gpu.py (atol 3e-2,
rtol 2e-2) against the CPU form of the same op; for fp8 / mxfp4 torch.equal with the packed-bf16
launch over the dequantised weight; and native().gemm_tile_plan reports the walked row, the schedule
that ran and the grid the shapes give."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from test_gemm_tile_f4_gpu import _w as _w4, _w13 as _w13_4
from test_gemm_tile_f8_gpu import _close, _cs, _ss, _w as _w8, _w13 as _w13_8, _x

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
M = 300
COUNTS = (0, 300, 45)  # grouped: rows per expert, after 8 rows of no expert and before 7 more
ROWS_G = sum(COUNTS) + 15
BF16, SWIGLU, ROPE, RESID, SWIGLU8 = range(5)


def _guarded(rows, cols, dtype=torch.bfloat16):
    """A NaN-filled [rows + 1, cols] buffer: its first rows are the output, the last is the guard."""
    return torch.full((rows + 1, cols), NAN, device=DEV, dtype=dtype)


def _weights(fmt, epi, N, K):
    """(bf16 weight [N, K] the CPU form reads, the tensors to launch as ((w, wscale), ...))."""
    src = (_w13_4 if fmt == 2 else _w13_8) if epi == SWIGLU8 else (_w4 if fmt == 2 else _w8)
    dq, qp, s = src(N // 2, K) if epi == SWIGLU8 else src(N, K)
    if fmt:
        return dq, ((qp, s),)
    return dq, ((dq, None), (ops.pack_skinny(dq), None))


def _plan_is(row, K, algo, sch, E, N):
    fmt, epi, grouped, rs, _ = ops.TILE_FORMS[row]
    rows = ROWS_G if grouped else M
    err, psch, form, n_mt, n_nt, nwg = ops.native().gemm_tile_plan(fmt, rows, N, K, epi, algo, E, K // 128 if rs else 0)
    assert (err, psch, form) == (0, sch, row)
    assert n_mt * n_nt == nwg == ((rows + 255) // 256 + E) * ((N + 255) // 256)


@pytest.mark.parametrize("row", range(len(ops.TILE_FORMS)), ids=lambda r: "fmt%d-epi%d-g%d-rs%d-sch0_%d" % ops.TILE_FORMS[r])
def test_every_form_launches(row):
    fmt, epi, grouped, rs, sch0 = ops.TILE_FORMS[row]
    swg = epi in (SWIGLU, SWIGLU8)
    N = 512 if swg else 384
    # (K, algo asked for, schedule that runs)
    runs = [(512 if rs else 256, 1, 1)] + ([(256, 0, 0), (128, 1, 0)] if sch0 else [])
    for K, algo, sch in runs:
        what = f"row {row} {ops.TILE_FORMS[row]} K={K} algo={algo}"
        _plan_is(row, K, algo, sch, 3 if grouped else 0, N)
        dq, launches = _weights(fmt, epi, N, K)
        if grouped:
            _grouped(epi, N, K, algo, dq, what)
        elif epi == RESID:
            _resid(N, K, dq, launches, what)
        else:
            _dense(epi, rs, N, K, algo, dq, launches, what)


def _dense(epi, rs, N, K, algo, dq, launches, what):
    x = _x(M, K)
    kw = {}
    if epi == ROPE:
        kw["rope"] = (((torch.arange(M, device=DEV) * 37 + 11) % 4096).to(torch.int32), _cs(), 2)
    elif epi != BF16:
        kw["swiglu"] = 8 if epi == SWIGLU8 else True
    if rs:
        kw["rowscale"] = (_ss(M, K), 1e-5)
    cpu = {k: (tuple(t.cpu() if torch.is_tensor(t) else t for t in v) if isinstance(v, tuple) else v) for k, v in kw.items()}
    r32 = ops.gemm_tile(x.cpu(), dq.cpu(), algo=algo, **cpu)
    for w, s in launches:
        buf = _guarded(M, r32.shape[1])
        y = ops.gemm_tile(x, w, algo=algo, out=buf[:M], wscale=s, **kw)
        assert y.data_ptr() == buf.data_ptr() and not torch.isnan(buf[:M]).any(), f"{what}: a due store is missing"
        assert torch.isnan(buf[M]).all(), f"{what}: the guard row was written"
        _close(y.cpu(), r32, what)
        if s is not None:
            assert torch.equal(y, ops.gemm_tile(x, ops.pack_skinny(dq), algo=algo, **kw)), f"{what}: differs from bf16"


def _resid(N, K, dq, launches, what):
    x = _x(M, K)
    g = torch.Generator(device=DEV).manual_seed(N + M)
    resid = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    nw = (torch.rand(N, device=DEV, generator=g) + 0.5).to(torch.bfloat16)
    rc = resid.cpu().clone()
    hc, sc = ops.gemm_tile_resid(x.cpu(), dq.cpu(), rc, nw.cpu())
    for w, s in launches:
        rbuf, hbuf, sbuf = _guarded(M, N), _guarded(M, N), _guarded(M, N // 128, torch.float32)
        rbuf[:M] = resid
        h, ss = ops.gemm_tile_resid(x, w, rbuf[:M], nw, hw=hbuf[:M], ss=sbuf[:M], wscale=s)
        for buf, ref_, name in ((rbuf, rc, "resid"), (hbuf, hc, "hw"), (sbuf, sc, "ss")):
            assert not torch.isnan(buf[:M]).any(), f"{what}: a due store of {name} is missing"
            assert torch.isnan(buf[M]).all(), f"{what}: the guard row of {name} was written"
            _close(buf[:M].cpu(), ref_, f"{what} {name}")
        if s is not None:
            rb = resid.clone()
            hb, sb = ops.gemm_tile_resid(x, ops.pack_skinny(dq), rb, nw)
            assert torch.equal(rbuf[:M], rb) and torch.equal(h, hb) and torch.equal(ss, sb), f"{what}: differs from bf16"


def _grouped(epi, N, K, algo, dq, what):
    E, lead, rows = len(COUNTS), 8, ROWS_G
    x = _x(rows, K)
    off = torch.tensor([lead, lead, lead + 300, lead + 345], dtype=torch.int32)
    assert off.diff().tolist() == list(COUNTS) and off[-1] < rows
    # expert e reads the weight's rows rotated by 16 e: three different weights with one construction
    w3 = torch.stack([dq.roll(16 * e, 0) for e in range(E)]).contiguous()
    swiglu = 8 if epi == SWIGLU8 else epi == SWIGLU
    ncol = N // 2 if swiglu else N
    r32 = ops.gemm_tile(x.cpu(), w3.cpu(), off, swiglu=swiglu, algo=algo,
                        out=torch.full((rows, ncol), NAN, dtype=torch.bfloat16))
    inside = torch.zeros(rows, dtype=torch.bool)
    inside[lead:lead + 345] = True
    assert torch.isnan(r32[~inside]).all() and not torch.isnan(r32[inside]).any()
    for w in (w3, torch.stack([ops.pack_skinny(e) for e in w3])):
        buf = _guarded(rows, ncol)
        y = ops.gemm_tile(x, w, off.to(DEV), swiglu=swiglu, algo=algo, out=buf[:rows]).cpu()
        assert not torch.isnan(y[inside]).any(), f"{what}: a due store is missing"
        assert torch.isnan(y[~inside]).all(), f"{what}: a row of no expert was written"
        assert torch.isnan(buf[rows]).all(), f"{what}: the guard row was written"
        _close(y[inside], r32[inside], what)
