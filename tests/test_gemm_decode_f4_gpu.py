"""The mxfp4-weight instantiations of the shared-A decode GEMM (ops.DEC_F4_FORMS), with the shapes of
tests/test_gemm_decode_f8_gpu.py: K = 512; rows 1, 16 * min(max m-tiles, 4), 65 and 16 * max
m-tiles (the last two above 4 m-tiles); N ragged in the last workgroup; splits 1, and 2 for the
SLAB forms of depth 8; NaN-filled outputs.

Weight element (r, k) is multiplied by 2^((r + k // 32) % 7 - 3) before quantising, so
neighbouring rows and neighbouring k-blocks carry different scales: a scale read in the wrong row
order, the wrong block or the wrong gate / up half cannot pass.  Per launch:
  1. bit equality (torch.equal) with the bf16 dec_gemm of the same configuration over
     pack_skinny(dequantised weights) - SLAB slab by slab: code * 2^e converts to bf16 exactly and
     the MFMA sequence and the epilogue are the bf16 ones;
  2. the project's bound against the fp32 product over the dequantised weights
     (2.5e-2 * scale + 1e-3; 3e-2 with the deferred norm)."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F_ = torch.nn.functional
K = 512
F4_FORMS = [ops.DEC_FORMS[i] for i, _ in ops.DEC_F4_FORMS]
_ID = "epi{}-ntw{}-w{}-d{}-mt{}-wide{}"


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    _w.cache_clear()
    _w13.cache_clear()


def _check(y, ref, what, tol=2.5e-2):
    err = (y.float() - ref.float()).abs().max().item()
    scale = ref.float().abs().max().item()
    print(f"{what}: max err {err:.4g} scale {scale:.4g}")
    assert err <= tol * scale + 1e-3, f"{what}: max err {err:.4g} vs scale {scale:.4g}"


def _quant(w):
    """(dequantised bf16 [N, K], packed codes, packed scales) of a row-major weight in its packed row order."""
    c, s = ops.quantize_mxfp4(w)
    return (ops.dequantize_mxfp4(c, s),) + ops.pack_skinny_f4(c, s)


def _spread(N):
    """2^((r + k // 32) % 7 - 3): another scale in every neighbouring row and k-block."""
    r, b = torch.arange(N, device=DEV)[:, None], torch.arange(K, device=DEV)[None, :] // 32
    return torch.exp2(((r + b) % 7 - 3).float())


@functools.lru_cache(maxsize=None)
def _w(N, seed=0):
    g = torch.Generator(device=DEV).manual_seed(2000 + seed)
    w = torch.randn(N, K, device=DEV, generator=g) * 0.02 * _spread(N)
    return _quant(w.to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def _w13(F):
    """gate / up weights of F features each: the dequantised [gate; up], and the packed encodings of
    the [8 gate | 8 up] interleaved rows (the scales permuted with them)."""
    gu = torch.cat([_w(F, 1)[0], _w(2 * F, 2)[0][F:]])  # up rows F.. of another draw: other scales than gate's
    il = ops.interleave_gate_up8(gu)
    dq, cp, sp = _quant(il)
    assert torch.equal(dq, il), "dequantised values are stable under re-quantisation"
    return gu, ops.pack_skinny(il), cp, sp


def _x(M):
    g = torch.Generator(device=DEV).manual_seed(M * 7919 + K)
    return torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)


def _launch(epi, cfg, N, M, a, f4, rownorm=None):
    """One dec_gemm launch over NaN-filled outputs, over the mxfp4 (``f4``) or the bf16 encoding of
    the same weights; returns the raw output: SLAB [S, M, N] fp32, BF16 [M, N], SWIGLU8 [M, N / 2]."""
    S = cfg[0]
    if epi == ops.DEC_SWIGLU8:
        _, wp, cp, sp = _w13(N // 2)
    else:
        dq, cp, sp = _w(N)
        wp = ops.pack_skinny(dq)
    kw = dict(wscale=sp) if f4 else {}
    w = cp if f4 else wp
    if epi == ops.DEC_SLAB:
        ws = torch.full((S * M * N + 64,), float("nan"), device=DEV, dtype=torch.float32)
        assert ops.dec_gemm(a, w, epi, M, workspace=ws, rownorm=rownorm, cfg=cfg, **kw) == S
        assert not torch.isnan(ws[: S * M * N]).any(), "every slab element written"
        assert torch.isnan(ws[S * M * N:]).all(), "nothing written past the slabs"
        return ws[: S * M * N].view(S, M, N)
    if epi == ops.DEC_BF16:
        y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        ops.dec_gemm(a, w, epi, M, out=y, rownorm=rownorm, cfg=cfg, **kw)
        assert not torch.isnan(y).any(), "every column of every row written (the ragged last workgroup included)"
        return y
    act = torch.full((-(-M // 16), N // 64, 64, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.dec_gemm(a, w, epi, M, out=act, rownorm=rownorm, cfg=cfg, **kw)
    y = ops.unpack_skinny(act)[:M]
    assert not torch.isnan(y).any(), "every feature of every row written"
    return y


def _ref(epi, N, xf):
    """The fp32 product of rows xf [M, K] over the dequantised weights (SWIGLU8: gate and up rounded
    to bf16 first, as the kernel)."""
    if epi != ops.DEC_SWIGLU8:
        return xf @ _w(N)[0].float().t()
    gu = _w13(N // 2)[0].float()
    g = (xf @ gu[: N // 2].t()).to(torch.bfloat16).float()
    u = (xf @ gu[N // 2:].t()).to(torch.bfloat16).float()
    return F_.silu(g) * u


def _both(epi, cfg, N, M, a, ref, what, rownorm=None, tol=2.5e-2):
    y4 = _launch(epi, cfg, N, M, a, True, rownorm)
    yb = _launch(epi, cfg, N, M, a, False, rownorm)
    same = torch.equal(y4, yb)
    diff = (y4.float() - yb.float()).abs().max().item()
    print(f"{what}: mxfp4 vs bf16 launch bit-equal {same}, max diff {diff:.4g}")
    assert same, f"{what}: the mxfp4 launch differs from the bf16 launch over the dequantised weights (max {diff:.4g})"
    _check(y4.sum(0) if epi == ops.DEC_SLAB else y4, ref, what, tol)


def _shape_n(epi, ntw, waves):
    return 64 * (waves + 1) if epi == ops.DEC_SWIGLU8 else 16 * (2 * ntw * waves + 1)


@pytest.mark.parametrize("form", F4_FORMS, ids=lambda f: _ID.format(*f))
def test_f4_form_bit_equal_to_bf16_and_within_bound(form):
    epi, ntw, waves, depth, max_mt, _ = form
    N = _shape_n(epi, ntw, waves)
    rows = [1, 16 * min(max_mt, 4)] + ([65, 16 * max_mt] if max_mt > 4 else [])
    splits = [1, 2] if epi == ops.DEC_SLAB and depth == 8 else [1]
    for M in rows:
        x = _x(M)
        ref = _ref(epi, N, x.float())
        for S in splits:
            _both(epi, (S, ntw, waves, depth), N, M, ops.pack_activation(x), ref, f"{form} M{M} S{S}")
    if max_mt == 4:  # no 5 m-tile instantiation: refused by the table, before any launch
        with pytest.raises(RuntimeError, match="not compiled for 65 rows over mxfp4 weights"):
            _launch(epi, (1, ntw, waves, depth), N, 65, ops.pack_activation(_x(65)), True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", F4_FORMS, ids=lambda f: _ID.format(*f))
def test_f4_form_narrow_deferred_norm(form):
    """The deferred RMSNorm over per-512-column sums of squares (what add_norm_partial leaves), rows
    of very different norms: another row's 1/rms cannot pass the bound."""
    epi, ntw, waves, depth, max_mt, _ = form
    N = _shape_n(epi, ntw, waves)
    nw = (torch.rand(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) + 0.5).to(torch.bfloat16)
    for M in [m for m in (1, 64, 128) if m <= 16 * max_mt]:
        res = (_x(M).float() * (1 + torch.arange(M, device=DEV).float() / 8).unsqueeze(1)).to(torch.bfloat16)
        ss = (res.float() ** 2).view(M, K // 512, 512).sum(-1).contiguous()
        xw = ops.pack_activation((res.float() * nw.float()).to(torch.bfloat16))
        xn = F_.rms_norm(res.float(), (K,), nw.float(), 1e-5)
        _both(epi, (1, ntw, waves, depth), N, M, xw, _ref(epi, N, xn), f"{form} narrow norm M{M}",
              rownorm=(ss, 1e-5), tol=3e-2)
    torch.cuda.synchronize()


def test_every_e2m1_code_converts_exactly_at_every_position_and_scale():
    """One weight whose rows run through all 16 codes at every nibble and byte position, with block
    scales that vary by row and block and include both clamp ends (bytes 67 and 187) and a block of
    zeros; one-hot activation rows select the k positions; the SLAB output must be the dequantised
    weight exactly (fp32 slabs: -0 against +0 aside, which compare equal)."""
    epi, ntw, waves, depth = ops.DEC_FORMS[ops.DEC_F4_FORMS[0][0]][:4]
    assert epi == ops.DEC_SLAB
    N, M = 16 * ntw * waves, 64
    n, k = torch.arange(N, device=DEV)[:, None], torch.arange(K, device=DEV)[None, :]
    nib = ((n * 5 + k * 3 + k // 16) % 16).to(torch.uint8)  # all 16 codes in every row at every k % 8
    for pos in range(8):
        assert all(nib[r, pos::8].unique().numel() == 16 for r in (0, N - 1))
    nib[3, 64:96] = 0  # a block of zeros
    codes = nib[:, 0::2] | (nib[:, 1::2] << 4)
    blk = torch.arange(K // 32, device=DEV)[None, :]
    sb = (127 + (n * 3 + blk * 7) % 13 - 6).to(torch.uint8)  # e in -6 .. 6, another in every row and block
    sb[0, 0], sb[1, 1], sb[N - 1, K // 32 - 1], sb[3, 2] = 67, 187, 187, 127  # both clamp ends; the zero block's 127
    want = ops.dequantize_mxfp4(codes, sb, torch.float32)
    assert torch.isfinite(want).all() and want.abs().max() == 6 * 2.0 ** 60 and want[3, 64:96].abs().max() == 0
    cp, sp = ops.pack_skinny_f4(codes, sb)
    for base in range(0, K, M):  # one-hot rows over every k position
        x = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
        x[torch.arange(M), base + torch.arange(M)] = 1
        ws = torch.full((M * N,), float("nan"), device=DEV, dtype=torch.float32)
        assert ops.dec_gemm(ops.pack_activation(x), cp, epi, M, workspace=ws, cfg=(1, ntw, waves, depth), wscale=sp) == 1
        got = ws.view(M, N)
        assert torch.equal(got, want[:, base:base + M].t()), \
            f"k {base}..{base + M - 1}: a code converted inexactly, out of place or with another block's scale"
    torch.cuda.synchronize()


def test_unsupported_mxfp4_launches_raise_and_take_no_other_path():
    """Grouped launches, the wide deferred norm, a form outside DEC_F4_FORMS, a K slice that is not
    whole F4 ring turns and a missing or misshapen scale tensor: an error, never another kernel."""
    out_forms = [f for i, f in enumerate(ops.DEC_FORMS) if i not in [j for j, _ in ops.DEC_F4_FORMS]]
    assert out_forms, "some form has no mxfp4 instantiation"
    for epi, ntw, waves, depth, _, _ in out_forms:
        N = _shape_n(epi, ntw, waves)
        with pytest.raises(RuntimeError, match="over mxfp4 weights"):
            _launch(epi, (1, ntw, waves, depth), N, 1, ops.pack_activation(_x(1)), True)
    epi, ntw, waves, depth = F4_FORMS[0][:4]
    N = _shape_n(epi, ntw, waves)
    _, cp, sp = _w(N)
    a = ops.pack_activation(_x(1))
    ws = torch.zeros(4 * N, device=DEV)
    with pytest.raises(ValueError, match="packed block scales"):
        ops.dec_gemm(a, cp, epi, 1, workspace=ws, cfg=(1, ntw, waves, depth))
    with pytest.raises(ValueError, match="packed block scales"):
        ops.dec_gemm(a, cp, epi, 1, workspace=ws, cfg=(1, ntw, waves, depth), wscale=sp.flatten())
    with pytest.raises(RuntimeError, match="over mxfp4 weights in 4 K slices"):  # 128-deep slices: half an A chunk
        ops.dec_gemm(a, cp, epi, 1, workspace=ws, cfg=(4, ntw, waves, depth), wscale=sp)
    wide = next(f for f in F4_FORMS if f[5])  # the form has a wide-norm instantiation over bf16 only
    Nw = _shape_n(wide[0], wide[1], wide[2])
    ss16 = torch.ones(1, 32, device=DEV)  # more than 16 partial sums per row: the wide deferred norm
    with pytest.raises(RuntimeError, match="wide deferred norm"):
        _launch(wide[0], (1,) + wide[1:4], Nw, 1, a, True, rownorm=(ss16, 1e-5))
    with pytest.raises(ValueError, match="no mxfp4 form"):
        ops.dec_gemm_grouped(a, cp[None], epi, 1, workspace=ws)
    assert not ops.dec_form_ok(epi, (1, ntw, waves, depth), 1, grouped=True, f4=True)
    assert not ops.dec_form_ok(wide[0], (1,) + wide[1:4], 1, wide_norm=True, f4=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry", ops.DEC_F4_FORMS, ids=lambda e: f"form{e[0]}-ring{e[1]}")
def test_every_f4_ring_depth_is_bit_equal_to_bf16(entry, monkeypatch):
    """The launcher takes an F4 ring of 8 k-steps, and at <= 16 rows the form's own depth (16)
    where it divides the K slice.  K = 1024 with 1 and 2 splits: every instantiated depth, chosen
    or forced (ops.DEC_F4_DEPTH_FORCE), must give the bf16 launch's bits at 1, 16 and 17 rows and
    at the form's most rows; a depth the rule does not reach is refused."""
    idx, d1 = entry
    epi, ntw, waves, depth, max_mt, _ = ops.DEC_FORMS[idx]
    K1, N = 1024, _shape_n(epi, ntw, waves)
    g = torch.Generator(device=DEV).manual_seed(77 + idx)
    r, b = torch.arange(N, device=DEV)[:, None], torch.arange(K1, device=DEV)[None, :] // 32
    w = torch.randn(N, K1, device=DEV, generator=g) * 0.02 * torch.exp2(((r + b) % 7 - 3).float())
    c, s = ops.quantize_mxfp4(w.to(torch.bfloat16))  # SWIGLU8: taken as the [8 gate | 8 up] rows
    (cp, sp), wp = ops.pack_skinny_f4(c, s), ops.pack_skinny(ops.dequantize_mxfp4(c, s))

    def run(wgt, M, a, S, **kw):
        cfg = (S, ntw, waves, depth)
        if epi == ops.DEC_SLAB:
            out = torch.full((S * M * N,), float("nan"), device=DEV)
            assert ops.dec_gemm(a, wgt, epi, M, workspace=out, cfg=cfg, **kw) == S
        elif epi == ops.DEC_BF16:
            out = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
            ops.dec_gemm(a, wgt, epi, M, out=out, cfg=cfg, **kw)
        else:
            out = torch.full((-(-M // 16), N // 64, 64, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
            ops.dec_gemm(a, wgt, epi, M, out=out, cfg=cfg, **kw)
            out = ops.unpack_skinny(out)[:M]
        assert not torch.isnan(out).any()
        return out

    for M in sorted({1, 16, 17, 16 * max_mt}):
        a = ops.pack_activation(torch.randn(M, K1, device=DEV, generator=g).to(torch.bfloat16))
        for S in ((1, 2) if epi == ops.DEC_SLAB else (1,)):
            monkeypatch.setattr(ops, "DEC_F4_DEPTH_FORCE", 0)
            want = run(wp, M, a, S)
            for d in (0, 8, 16, 32):
                monkeypatch.setattr(ops, "DEC_F4_DEPTH_FORCE", d)
                if d in (0, 8) or (d == 16 and d1 >= 16 and M <= 16):
                    assert torch.equal(run(cp, M, a, S, wscale=sp), want), f"ring depth {d} at {M} rows, {S} splits"
                else:
                    with pytest.raises(RuntimeError, match="not compiled"):
                        run(cp, M, a, S, wscale=sp)
    torch.cuda.synchronize()
