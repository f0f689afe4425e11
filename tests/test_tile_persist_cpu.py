"""The persistent form of the prefill tile GEMM, without a launch: ops.TILE_PERSIST_FORMS against
kTilePersist (ops/csrc/gemm_tile_forms.h) through native().gemm_tile_persist_forms, and tile_plan's
routing - which launches run persistent and on what grid - through native().gemm_tile_plan(ext=True).
The cases that ask the extension skip where it is not built."""
import pytest

from k8s_llm_monitor_amd import ops

BF16, SWIGLU, ROPE, RESID, SWIGLU8 = range(5)
M = 16384  # the headline's prefill step: 64 m-tiles


def _plan(fmt, M_, N, K, epi, sch=1, E=0, rs_np=0, **kw):
    if not ops.native_available():
        pytest.skip("the extension is not built")
    r = ops.native().gemm_tile_plan(fmt, M_, N, K, epi, sch, E, rs_np, ext=True, **kw)
    return dict(zip(("err", "sch", "form", "n_mt", "n_nt", "nwg", "persist", "grid"), r))


def test_side_table_is_the_headers():
    rows = ops.TILE_PERSIST_FORMS
    assert len(set(r[:2] for r in rows)) == len(rows)
    # every persistent instantiation is a dense bf16 row of the table of forms
    assert all((0, epi, 0, rs) in {f[:4] for f in ops.TILE_FORMS} for epi, rs, _ in rows)
    if not ops.native_available():
        pytest.skip("the extension is not built")
    assert [tuple(r) for r in ops.native().gemm_tile_persist_forms()] == list(rows)


def test_default_plan_is_unchanged_in_its_first_six():
    if not ops.native_available():
        pytest.skip("the extension is not built")
    plan = ops.native().gemm_tile_plan
    six = plan(0, M, 4096, 4096, RESID, 1, 0, 0)
    assert len(six) == 6 and list(plan(0, M, 4096, 4096, RESID, 1, 0, 0, ext=True))[:6] == list(six)
    assert six[5] == 64 * 16  # nwg stays the tile count, persistent or not


@pytest.mark.parametrize("epi,rs_np,N,K", [(ROPE, 32, 6144, 4096), (RESID, 0, 4096, 4096), (SWIGLU8, 32, 28672, 4096),
                                           (RESID, 0, 4096, 14336)])
def test_headline_launches(epi, rs_np, N, K):
    """The four launches of the fused-norm prefill layer: persistent exactly where the side table says."""
    pi = [r[:2] for r in ops.TILE_PERSIST_FORMS].index((epi, int(rs_np > 0)))
    on = ops.TILE_PERSIST_FORMS[pi][2]
    tiles = 64 * (N // 256)
    p = _plan(0, M, N, K, epi, rs_np=rs_np)
    assert (p["err"], p["sch"], p["nwg"]) == (0, 1, tiles)
    assert (p["persist"], p["grid"]) == ((pi, 256) if on else (-1, tiles))
    # the A/B override, and the grid of another device
    assert _plan(0, M, N, K, epi, rs_np=rs_np, persist=0)["persist"] == -1
    p = _plan(0, M, N, K, epi, rs_np=rs_np, persist=1, cus=304)
    assert (p["persist"], p["grid"], p["nwg"]) == (pi, 304, tiles)
    p = _plan(0, M, N, K, epi, rs_np=rs_np, persist=1, cus=3)
    assert (p["persist"], p["grid"]) == (pi, 3)


def test_everything_else_stays_one_tile():
    """Forced on, the persistent form still runs only where it is compiled and has something to walk."""
    def one_tile(p):
        return p["err"] == 0 and p["persist"] == -1 and p["grid"] == p["nwg"]
    kw = dict(persist=1)
    assert one_tile(_plan(0, 1024, 4096, 4096, RESID, **kw))             # 64 tiles <= 256 CUs
    assert one_tile(_plan(0, 16 * 256, 16 * 256, 4096, RESID, **kw))     # exactly one tile per CU
    assert _plan(0, 16 * 256 + 1, 16 * 256, 4096, RESID, **kw)["persist"] >= 0
    assert one_tile(_plan(0, M, 4096, 4096, BF16, **kw))                 # rows of the table without a persistent form
    assert one_tile(_plan(0, M, 4096, 4096, ROPE, **kw))
    assert one_tile(_plan(0, M, 4096, 4096, SWIGLU8, **kw))
    assert one_tile(_plan(0, M, 4096, 4096, SWIGLU, rs_np=32, **kw))
    assert one_tile(_plan(0, M, 4096, 4096, SWIGLU8, E=8, **kw))         # grouped
    assert one_tile(_plan(0, M, 4096, 128, ROPE, sch=1, **kw))           # K < 192: schedule 0
    assert one_tile(_plan(0, M, 4096, 4096, SWIGLU8, sch=0, **kw))
    for fmt in (1, 2):                                                   # fp8, mxfp4
        assert one_tile(_plan(fmt, M, 4096, 4096, RESID, **kw))
        assert one_tile(_plan(fmt, M, 4096, 4096, SWIGLU8, rs_np=32, **kw))
    assert _plan(0, M, 4096, 192, RESID, **kw)["persist"] >= 0           # three k-tiles: the least
    assert one_tile(_plan(0, M, 4096, 4096, RESID, persist=1, cus=0))    # no CU count, no persistent grid
    p = _plan(0, 0, 4096, 4096, RESID, **kw)                             # an empty launch
    assert (p["err"], p["persist"], p["grid"]) == (0, -1, 0)
    assert _plan(0, M, 4096 + 8, 4096, RESID, **kw)["err"] == -1         # a refused launch stays refused


def test_module_constants_default_to_the_table():
    assert ops.TILE_PERSIST == -1 and ops.TILE_PERSIST_CUS == 0
