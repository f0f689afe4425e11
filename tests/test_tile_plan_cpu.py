"""The prefill tile GEMM's table of forms and its launch plan, without a launch: ops.TILE_FORMS and
ops.tile_form_why (the Python copy the CPU path refuses with) against kTileForms and tile_plan of
ops/csrc/gemm_tile_forms.h, through native().gemm_tile_forms / gemm_tile_plan.  The cases that ask
the extension skip where it is not built; the rule function's own answers need nothing."""
import itertools

import pytest

from k8s_llm_monitor_amd import ops

BF16, SWIGLU, ROPE, RESID, SWIGLU8 = range(5)
NS = (16, 24, 128, 256, 384, 400, 512)
KS = (64, 128, 192, 256, 320, 384)
# the 32-bit boundaries tests/test_prefill_f8_cpu.py and test_prefill_f4_cpu.py pin
BOUNDARY = ((1 << 16, 1 << 15), ((1 << 16) - 16, 1 << 16), (1 << 16, 1 << 16))


def _plan(enc, M, N, K, epi, sch, E=0, rs_np=0):
    if not ops.native_available():
        pytest.skip("the extension is not built")
    r = ops.native().gemm_tile_plan(ops.TILE_ENCS.index(enc), M, N, K, epi, sch, E, rs_np)
    return dict(zip(("err", "sch", "form", "n_mt", "n_nt", "nwg"), r))


def test_table_is_the_headers():
    assert len(ops.TILE_FORMS) == 23 and sum(1 + f[4] for f in ops.TILE_FORMS) == 30
    assert len(set(f[:4] for f in ops.TILE_FORMS)) == len(ops.TILE_FORMS)
    if not ops.native_available():
        pytest.skip("the extension is not built")
    assert [tuple(r) for r in ops.native().gemm_tile_forms()] == list(ops.TILE_FORMS)


def test_plan_accepts_exactly_what_the_rule_does():
    """err == 0 exactly where ops.tile_form_why finds a form; an accepted plan names the row."""
    if not ops.native_available():
        pytest.skip("the extension is not built")
    plan = ops.native().gemm_tile_plan
    n = n_ok = 0
    shapes = list(itertools.product(NS, KS))
    for fmt, enc in enumerate(ops.TILE_ENCS):
        extra = [BOUNDARY[0]] if enc == "fp8" else list(BOUNDARY[1:]) if enc == "mxfp4" else list(BOUNDARY)
        for epi, E, rs_np, sch, (N, K) in itertools.product(range(-1, 6), (0, 1, 256, 257), (0, 4, 6, 8, 64, 68),
                                                           (-1, 0, 1, 2), shapes + extra):
            err, psch, form = plan(fmt, 300, N, K, epi, sch, E, rs_np)[:3]
            why = ops.tile_form_why(enc, epi, E, rs_np, sch, N, K)
            assert (err == 0) == (why is None), (enc, epi, E, rs_np, sch, N, K, err, why)
            n += 1
            if err == 0:
                n_ok += 1
                assert ops.TILE_FORMS[form][:4] == (fmt, epi, int(E > 0), int(rs_np > 0))
                assert psch == (sch if K >= 192 else 0) and (psch == 1 or ops.TILE_FORMS[form][4])
    print(f"{n} requests, {n_ok} accepted")
    assert n_ok > 0


def test_pinned_refusal_codes():
    assert _plan("bf16", 300, 24, 256, BF16, 1)["err"] == -1                         # N % 16
    assert _plan("bf16", (1 << 31) - 256, (1 << 24) - 16, 64, BF16, 0)["err"] == -2   # 2^39 tiles
    assert _plan("fp8", 300, 1 << 16, 1 << 15, BF16, 1)["err"] == -3                  # 2^31 bytes of codes
    assert _plan("mxfp4", 300, 1 << 16, 1 << 16, BF16, 1)["err"] == -3
    assert _plan("mxfp4", 300, (1 << 16) - 16, 1 << 16, BF16, 1)["err"] == 0
    assert _plan("bf16", 300, 256, 256, RESID, 1)["err"] == 0
    assert _plan("bf16", 300, 1 << 22, 64, RESID, 1)["err"] == -1                     # K < 192 comes first
    assert _plan("bf16", 300, 1 << 22, 192, RESID, 1)["err"] == -3                    # 256 rows of the residual
    assert _plan("fp8", 300, 256, 256, SWIGLU, 1)["err"] == -4                        # no per-128 pairing
    assert _plan("fp8", 300, 256, 256, BF16, 0)["err"] == -4                          # schedule 1 only
    assert _plan("mxfp4", 300, 256, 320, BF16, 1)["err"] == -4                        # K % 128
    assert _plan("fp8", 300, 256, 256, BF16, 1, E=2)["err"] == -4                     # dense only
    # -4 before -1: a quantised request that is wrong twice
    assert _plan("fp8", 300, 24, 128, BF16, 1)["err"] == -4
    assert _plan("fp8", 300, 24, 256, BF16, 1)["err"] == -1
    assert _plan("fp8", 300, 256, 256, 7, 1)["err"] == -1 and _plan("fp8", 300, 256, 256, 7, 0)["err"] == -4
    # no rows: an empty launch of any form of a known format
    assert _plan("fp8", 0, 24, 128, SWIGLU, 0)["err"] == 0
    if ops.native_available():
        assert ops.native().gemm_tile_plan(3, 0, 256, 256, 0, 1, 0, 0)[0] == -4
        assert ops.native().gemm_tile_plan(-1, 300, 256, 256, 0, 1, 0, 0)[0] == -4


def test_bf16_schedule_fallback():
    """Below K = 192 (three k-tiles) a schedule-1 request runs schedule 0 - where the form has it."""
    for K in (64, 128):
        for epi, N, E in ((BF16, 16, 0), (SWIGLU, 256, 0), (SWIGLU8, 256, 0), (ROPE, 128, 0), (BF16, 16, 3), (SWIGLU, 256, 3)):
            p = _plan("bf16", 300, N, K, epi, 1, E)
            assert (p["err"], p["sch"]) == (0, 0), (K, epi, E)
        assert _plan("bf16", 300, 128, K, RESID, 1)["err"] == -1
        for epi in (SWIGLU, SWIGLU8, ROPE):
            assert _plan("bf16", 300, 256, K, epi, 1, rs_np=4)["err"] == -1
    for epi, rs_np in ((BF16, 0), (RESID, 0), (ROPE, 4), (SWIGLU8, 4)):
        p = _plan("bf16", 300, 256, 192, epi, 1, rs_np=rs_np)
        assert (p["err"], p["sch"]) == (0, 1)
    p = _plan("bf16", 300, 256, 192, BF16, 0)
    assert (p["err"], p["sch"]) == (0, 0)
    assert _plan("bf16", 300, 256, 192, RESID, 0)["err"] == -1
    # the grid: two m-tiles (+ E for a grouped launch: the bound over any split of the rows), n-tiles rounded up
    p = _plan("bf16", 300, 384, 256, BF16, 1, E=3)
    assert (p["n_mt"], p["n_nt"], p["nwg"]) == (5, 2, 10)


def test_rule_alone():
    """No extension: the boundaries of the tile_*_ok fronts (the fp8 / mxfp4 ones are asserted in
    tests/test_prefill_f8_cpu.py and test_prefill_f4_cpu.py) and the bf16 rows of the rule."""
    why = ops.tile_form_why
    assert ops.tile_f8_ok(16, 192) and not ops.tile_f8_ok(16, 128) and not ops.tile_f8_ok(8, 256)
    assert ops.tile_f4_ok(16, 256) and not ops.tile_f4_ok(16, 192) and not ops.tile_f4_ok(16, 320)
    M = ops.TILE_MIN_M
    assert ops.tile_shape_ok(M, 16, 128) and not ops.tile_shape_ok(M - 1, 16, 128)
    assert not ops.tile_shape_ok(M, 16, 64) and not ops.tile_shape_ok(M, 8, 128) and not ops.tile_shape_ok(M, 16, 160)
    assert ops.tile_shape_ok(M, 256, 128, swiglu=True) and not ops.tile_shape_ok(M, 128, 128, swiglu=True)
    assert ops.tile_shape_ok(M, 1 << 14, (1 << 16) - 64) and not ops.tile_shape_ok(M, 1 << 14, 1 << 16)  # 2^31 bytes of W
    # bf16: K from 64 on, both schedules; the fused-norm forms on schedule 1 from K = 192 on
    for sch in (0, 1):
        assert why("bf16", BF16, 0, 0, sch, 16, 64) is None and why("bf16", BF16, 2, 0, sch, 16, 64) is None
        assert why("bf16", ROPE, 0, 0, sch, 128, 64) is None and "128" in why("bf16", ROPE, 0, 0, sch, 192, 64)
    assert why("bf16", BF16, 0, 0, 1, 16, 32) is not None and why("bf16", BF16, 0, 0, 2, 16, 64) is not None
    assert why("bf16", RESID, 0, 0, 1, 128, 192) is None and "schedule" in why("bf16", RESID, 0, 0, 0, 128, 192)
    assert "schedule" in why("bf16", RESID, 0, 0, 1, 128, 128)
    assert why("bf16", SWIGLU, 0, 4, 1, 256, 512) is None and "schedule" in why("bf16", SWIGLU, 0, 4, 0, 256, 512)
    assert why("bf16", SWIGLU, 0, 6, 1, 256, 768) is not None and why("bf16", SWIGLU, 0, 68, 1, 256, 8704) is not None
    assert "row scale" in why("bf16", BF16, 0, 4, 1, 256, 512) and "row scale" in why("bf16", RESID, 0, 4, 1, 256, 512)
    assert "dense" in why("bf16", ROPE, 2, 0, 1, 128, 256) and "dense" in why("bf16", SWIGLU, 2, 4, 1, 256, 512)
    assert why("bf16", BF16, 256, 0, 1, 16, 64) is None and "experts" in why("bf16", BF16, 257, 0, 1, 16, 64)
    # codes: dense, schedule 1, no per-128 SwiGLU pairing
    for enc, K in (("fp8", 192), ("mxfp4", 256)):
        assert why(enc, SWIGLU8, 0, 4, 1, 256, 512) is None and why(enc, RESID, 0, 0, 1, 128, K) is None
        assert "grouped" in why(enc, BF16, 1, 0, 1, 16, K) and "swiglu=1" in why(enc, SWIGLU, 0, 0, 1, 256, K)
        assert "schedule" in why(enc, BF16, 0, 0, 0, 16, K) and "K=128" in why(enc, BF16, 0, 0, 1, 16, 128)
