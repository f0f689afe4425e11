"""Paged decode attention's table of forms and its launch plan, without a launch: ops.PD_FORMS and
ops.paged_decode_why (the Python copy the model and the engine choose by) against kPdForms and
pd_plan of ops/csrc/paged_decode_forms.h, through native().paged_decode_forms / paged_decode_plan.
The cases that ask the extension skip where it is not built; the rule function's own answers need
nothing."""
import itertools

import pytest

from k8s_llm_monitor_amd import ops

FIELDS = ("err", "form", "tw", "merge", "reduce", "gx", "gy", "gz")


def _plan(D, Hq, Hkv, B, S, fused=False, f8=False, merge=False, tw_force=0):
    if not ops.native_available():
        pytest.skip("the extension is not built")
    return dict(zip(FIELDS, ops.native().paged_decode_plan(D, Hq, Hkv, B, S, fused, f8, merge, tw_force)))


def test_table_is_the_headers():
    assert len(ops.PD_FORMS) == 22
    assert len(set(ops.PD_FORMS)) == len(ops.PD_FORMS)
    # a row stands for TW = 32 and 64, a fused row also for MERGE false and true
    assert sum(2 * (2 if fused else 1) for _, _, fused, _ in ops.PD_FORMS) == 60
    if not ops.native_available():
        pytest.skip("the extension is not built")
    assert [tuple(r) for r in ops.native().paged_decode_forms()] == list(ops.PD_FORMS)


def test_plan_accepts_exactly_what_the_rule_does():
    """err == 0 exactly where ops.paged_decode_why finds a form and S is in [1, 64] (or there is no
    row to launch for: B = 0); an accepted plan names the row."""
    if not ops.native_available():
        pytest.skip("the extension is not built")
    plan = ops.native().paged_decode_plan
    n = n_ok = 0
    for D, Hkv, G, fused, f8, S, merge, B in itertools.product((32, 64, 128, 256), (1, 2, 8), range(1, 18),
                                                               (False, True), (False, True), (0, 1, 2, 64, 65),
                                                               (False, True), (0, 1, 6, 64)):
        err, form, tw, mg, red, gx, gy, gz = plan(D, G * Hkv, Hkv, B, S, fused, f8, merge, 0)
        n += 1
        if B == 0:
            assert (err, form, gx, gy, gz) == (0, -1, 0, 0, 0)
            continue
        why = ops.paged_decode_why(D, G, fused, f8)
        assert (err == 0) == (why is None and 1 <= S <= 64), (D, Hkv, G, fused, f8, S, merge, B, err, why)
        if err == 0:
            n_ok += 1
            assert ops.PD_FORMS[form] == (D, G, int(fused), int(f8))
            assert (gx, gy, gz) == (S, Hkv, B) and tw in (32, 64)
            assert mg == int(fused and merge and S > 1) and red == int(S > 1 and not mg)
    print(f"{n} requests, {n_ok} accepted")
    assert n_ok > 0


def test_pinned_refusal_codes():
    assert _plan(128, 24, 8, 4, 1)["err"] == -1                          # G = 3
    assert _plan(128, 24, 8, 4, 1, f8=True)["err"] == -1
    assert _plan(128, 32, 2, 4, 1, fused=True)["err"] == -1              # fused G = 16: no row ...
    assert _plan(128, 32, 2, 4, 1, fused=True, f8=True)["err"] == -1
    assert _plan(128, 32, 2, 4, 1)["err"] == 0                           # ... the unfused kernel has it
    assert _plan(64, 32, 2, 4, 1)["err"] == -1                           # D = 64 stops at G = 8
    assert _plan(256, 8, 8, 4, 1)["err"] == -1
    assert _plan(128, 32, 8, 4, 0)["err"] == -2 and _plan(128, 32, 8, 4, 65)["err"] == -2
    assert _plan(128, 32, 8, 4, 64)["err"] == 0
    assert _plan(64, 32, 8, 4, 1, f8=True)["err"] == -3
    assert _plan(64, 32, 8, 4, 1, fused=True)["err"] == -3
    assert _plan(64, 24, 8, 4, 1, fused=True)["err"] == -3               # -3 before -1
    assert _plan(64, 32, 8, 4, 65, f8=True)["err"] == -2                 # -2 before -3
    assert _plan(128, 24, 8, 4, 65)["err"] == -2                         # ... and before -1
    # no rows: an empty launch of any form
    for D, G, fused, f8, S in ((128, 4, False, False, 1), (64, 3, True, True, 65), (256, 17, False, True, 0)):
        p = _plan(D, G * 8, 8, 0, S, fused, f8)
        assert (p["err"], p["form"]) == (0, -1)


def test_tw_by_grid_size_or_forced():
    # S * Hkv * B = 383 and 384
    assert _plan(128, 4, 1, 383, 1)["tw"] == 64 and _plan(128, 4, 1, 384, 1)["tw"] == 32
    assert _plan(128, 32, 8, 16, 3)["tw"] == 32 and _plan(128, 32, 8, 15, 3)["tw"] == 64   # 384, 360
    assert _plan(128, 32, 8, 64, 1, fused=True)["tw"] == 32 and _plan(128, 32, 8, 8, 4, fused=True)["tw"] == 64
    for B in (1, 64):
        assert _plan(128, 32, 8, B, 1, tw_force=32)["tw"] == 32
        assert _plan(128, 32, 8, B, 1, tw_force=64)["tw"] == 64
        for other in (-1, 0, 1, 16, 48, 128):
            assert _plan(128, 32, 8, B, 1, tw_force=other)["tw"] == (32 if B == 64 else 64)


def test_merge_and_reduce():
    for fused, merge in itertools.product((False, True), repeat=2):
        p = _plan(128, 32, 8, 4, 1, fused=fused, merge=merge)
        assert (p["err"], p["merge"], p["reduce"]) == (0, 0, 0)           # S = 1: neither
    p = _plan(128, 32, 8, 4, 3, fused=True, merge=True)
    assert (p["merge"], p["reduce"]) == (1, 0)
    p = _plan(128, 32, 8, 4, 3, fused=True, merge=False)
    assert (p["merge"], p["reduce"]) == (0, 1)
    for S in (2, 3, 64):                                                  # unfused never merges
        p = _plan(128, 32, 8, 4, S, fused=False, merge=True)
        assert (p["merge"], p["reduce"]) == (0, 1)
        p = _plan(128, 32, 8, 4, S, f8=True, merge=True)
        assert (p["merge"], p["reduce"]) == (0, 1)


def test_rule_alone():
    """No extension: the rule the model (fused or not) and the engine (fp8 cache or not) ask."""
    why = ops.paged_decode_why
    assert ops.MAX_SPLITS == 64
    for G in (1, 2, 4, 8):
        assert why(128, G, True, False) is None and why(128, G, True, True) is None
        assert why(64, G) is None and why(128, G) is None and why(128, G, f8=True) is None
    # fused: no G = 16, no D = 64; the unfused kernel has G = 16 at D = 128 only
    assert "16" in why(128, 16, True, False) and "16" in why(128, 16, True, True)
    assert why(128, 16) is None and why(128, 16, f8=True) is None and why(64, 16) is not None
    assert "head_dim 128" in why(64, 4, True, False)
    assert why(128, 3) is not None and why(128, 3, True) is not None and why(256, 4) is not None
    # fp8: D = 128 only, whatever the group (what the engine asks at construction)
    assert "head_dim 128" in why(64, 4, False, True) and "head_dim 128" in why(64, None, False, True)
    assert why(128, None, False, True) is None and why(128, None, True, True) is None
    assert why(128, 3, False, True) is not None
