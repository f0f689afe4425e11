"""dec_plan's slab-epilogue and split-placement fields (csrc/gemm_dec_forms.h: row-wide stores,
write-through, one split per XCD) against their mirror ops.dec_slab_plan, over the shapes of
tests/test_gemm_decode_slab_rows_gpu.py and the Llama-3-8B projections, for every setting of the three
switches; the placement map is a bijection wherever it is accepted and the identity elsewhere."""
import itertools

import pytest

from k8s_llm_monitor_amd import ops

SLAB_FORMS = [f for f in ops.DEC_FORMS if f[0] == ops.DEC_SLAB]
SETTINGS = list(itertools.product((-1, 0, 1), repeat=3))


def _shapes():
    for _, ntw, waves, depth, max_mt, _ in SLAB_FORMS:
        kstep = 512 if depth == 16 else 256
        for S in (1, 2, 4, 8, 16):
            for M in (1, 16, 17, 63, 64) + ((65, 128) if max_mt == 8 else ()):
                for N in (16 * waves * 2, 16 * (waves + 3), 16 * waves * 3, 16 * waves * 4):
                    yield M, N, kstep * S, (S, ntw, waves, depth)
    for M in (1, 64, 128):  # the headline's projections
        for N, K in ((6144, 4096), (4096, 4096), (4096, 14336)):
            yield M, N, K, ops.dec_config(N, K, ops.DEC_SLAB, rows=M)


def _native_plan(M, N, K, cfg, sw, experts=0, rw=False):
    p = ops.native().gemm_dec_plan(0, M, N, K, cfg[0], ops.DEC_SLAB, *cfg[1:], 0, experts, rw, 0, *sw)
    assert p[0] == 0, (M, N, K, cfg)
    return p


def test_plan_fields_match_the_mirror():
    n = 0
    for M, N, K, cfg in _shapes():
        for sw in SETTINGS:
            p = _native_plan(M, N, K, cfg, sw)
            assert tuple(p[10:13]) == ops.dec_slab_plan(M, N, cfg, sw=sw), (M, N, K, cfg, sw)
            if M <= ops.DEC_NARROW_MAX_M:
                g = _native_plan(M, N, K, cfg, sw, experts=3, rw=True)
                assert tuple(g[10:13]) == ops.dec_slab_plan(M, N, cfg, grouped=True, sw=sw)
                assert g[12] == 0, "grouped launches keep the identity placement"
            n += 1
    assert n > 1000


def test_switch_constants_reach_the_plan(monkeypatch):
    """The module constants are dec_slab_plan's defaults, and the short overload of gemm_dec_plan is
    the as-shipped plan."""
    M, N, K, cfg = 64, 4096, 4096, (8, 1, 8, 8)
    shipped = tuple(ops.native().gemm_dec_plan(0, M, N, K, cfg[0], 0, *cfg[1:], 0, 0, False, 0))
    assert shipped[10:13] == ops.dec_slab_plan(M, N, cfg) == ops.dec_slab_plan(M, N, cfg, sw=(-1, -1, -1))
    assert shipped[10:13] == ops.dec_slab_shipped(M) == (1, 1, 1)
    assert ops.dec_slab_shipped(16) == (0, 0, 1) and ops.dec_slab_shipped(17) == (1, 1, 1)
    assert (ops.DEC_SLAB_ROWS, ops.DEC_SLAB_WT, ops.DEC_XCD_SPLITS) == (-1, -1, -1)
    for sw in SETTINGS:
        for name, v in zip(("DEC_SLAB_ROWS", "DEC_SLAB_WT", "DEC_XCD_SPLITS"), sw):
            monkeypatch.setattr(ops, name, v)
        assert ops.dec_slab_plan(M, N, cfg) == tuple(_native_plan(M, N, K, cfg, sw)[10:13])
    assert ops.dec_slab_plan(M, N, cfg, sw=(0, 1, 0)) == (0, 0, 0), "write-through only on the row-wide stores"
    assert ops.dec_slab_plan(M, N, cfg, sw=(1, 1, 1)) == (1, 1, 1)
    assert ops.dec_slab_plan(16, N, cfg, sw=(1, 1, 1)) == (0, 0, 1), "one m-tile keeps the 4-byte stores"


def test_other_epilogues_have_no_slab_fields():
    for epi, cfg, N in ((ops.DEC_SWIGLU8, (1, 1, 7, 8), 28672), (ops.DEC_BF16, (1, 4, 8, 4), 128256)):
        p = ops.native().gemm_dec_plan(0, 64, N, 4096, 1, epi, *cfg[1:], 0, 0, False, 0, 1, 1, 1)
        assert p[0] == 0 and tuple(p[10:13]) == (0, 0, 0)


@pytest.mark.parametrize("S", [2, 4, 8])
def test_placement_is_a_bijection(S):
    for gx in range(1, 70):
        if not ops.dec_xcd_ok(gx, S):
            assert (gx * S) % 8
            continue
        cells = [ops.dec_xcd_map(L, S) for L in range(gx * S)]
        assert sorted(cells) == [(x, y) for x in range(gx) for y in range(S)], (gx, S)
        # workgroups that share an XCD (equal L % 8) share a split; an XCD takes one split only
        for c in range(8):
            assert {y for L, (_, y) in enumerate(cells) if L % 8 == c} == {c % S}


def test_fallbacks_are_identity():
    assert not any(ops.dec_xcd_ok(gx, S) for gx in range(1, 70) for S in (1, 3, 5, 6, 7, 16, 32))
    assert not ops.dec_xcd_ok(3, 2) and not ops.dec_xcd_ok(3, 4) and ops.dec_xcd_ok(3, 8)
    for M, N, K, cfg in _shapes():
        gx = -(-(N // 16) // (cfg[1] * cfg[2]))
        want = int(cfg[0] in (2, 4, 8) and gx * cfg[0] % 8 == 0)
        assert _native_plan(M, N, K, cfg, (0, 0, 1))[12] == want == ops.dec_slab_plan(M, N, cfg, sw=(0, 0, 1))[2]
    # the headline's three projections are all remapped
    for N, K in ((6144, 4096), (4096, 4096), (4096, 14336)):
        assert ops.dec_slab_plan(64, N, ops.dec_config(N, K, 0, rows=64), sw=(1, 1, 1)) == (1, 1, 1)
